"""Compute-op dispatch layer.

Exactly two execution paths, chosen by tensor placement:

* **CUDA (= ROCm/HIP) tensors** -> the hand-written CDNA4 HIP kernels in
  ``sparkagd_amd/csrc`` via the ctypes binding in ``hiplib.py``. If the
  extension is missing on a GPU machine this raises — there is deliberately
  NO silent eager/PyTorch fallback on GPU (the HIP path must be the path
  that runs).
* **CPU tensors** -> the plain-PyTorch oracles in ``reference.py`` (test/CI
  path; also the ground truth the kernels are validated against).

No Triton, no multi-backend dispatch beyond this placement switch.
"""

from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

from . import reference
from .reference import (
    LOSS_LOGISTIC,
    LOSS_LEAST_SQUARES,
    LOSS_HINGE,
    LOSS_SMOOTH_HINGE,
    PROX_SIMPLE,
    PROX_L1,
    PROX_SQUARED_L2,
    PROX_ELASTIC_NET,
)

_hip = None
_hip_err: Optional[str] = None


def _get_hip():
    """Load the HIP extension binding, raising loudly on GPU if unavailable."""
    global _hip, _hip_err
    if _hip is None and _hip_err is None:
        try:
            from . import hiplib

            hiplib.load()
            _hip = hiplib
        except Exception as e:  # noqa: BLE001 - record and re-raise at use site
            _hip_err = f"{type(e).__name__}: {e}"
    if _hip is None:
        raise RuntimeError(
            "sparkagd_amd HIP extension (libagd_hip.so) is required for GPU "
            "tensors but could not be loaded. Build it with "
            "`python -c 'import __graft_entry__; __graft_entry__.build()'` "
            f"from the repo root. Underlying error: {_hip_err}"
        )
    return _hip


def hip_available() -> bool:
    try:
        _get_hip()
        return True
    except RuntimeError:
        return False


def _use_hip(t: torch.Tensor) -> bool:
    if t.is_cuda:
        if os.environ.get("SPARKAGD_FORCE_REFERENCE") == "1":
            return False
        return True
    return False


def dense_eval(
    features: torch.Tensor,
    labels: torch.Tensor,
    w: torch.Tensor,
    loss_type: int,
    mask: Optional[torch.Tensor] = None,
    need_grad: bool = True,
    sample_weight: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    if _use_hip(features):
        return _get_hip().dense_eval(features, labels, w, loss_type, mask,
                                     need_grad, sample_weight)
    return reference.dense_eval(features, labels, w, loss_type, mask,
                                need_grad, sample_weight)


def csr_eval(
    rowptr: torch.Tensor,
    col: torch.Tensor,
    val: torch.Tensor,
    labels: torch.Tensor,
    w: torch.Tensor,
    loss_type: int,
    mask: Optional[torch.Tensor] = None,
    d: Optional[int] = None,
    csc=None,
    need_grad: bool = True,
    sample_weight: Optional[torch.Tensor] = None,
    csc_heavy=None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    if _use_hip(val):
        return _get_hip().csr_eval(rowptr, col, val, labels, w, loss_type, mask,
                                   d, csc, need_grad, sample_weight, csc_heavy)
    # the torch reference (sparse_csr @ / .t() @) is already deterministic
    return reference.csr_eval(rowptr, col, val, labels, w, loss_type, mask, d,
                              need_grad, sample_weight)


# Packed bf16 shards (packing.PackedDense): GPU only; DenseShard routes here
# when it holds a valid packed copy, HostStreamedDenseShard per packed chunk.
def dense_eval_packed(pk, labels, w, loss_type, mask=None, need_grad=True,
                      sample_weight=None):
    return _get_hip().dense_eval_packed(pk, labels, w, loss_type, mask,
                                        need_grad, sample_weight)


def dense_margins_packed(pk, v: torch.Tensor) -> torch.Tensor:
    return _get_hip().dense_margins_packed(pk, v)


def dense_eval_from_margins_packed(pk, margins, labels, loss_type, mask=None,
                                   need_grad=True, sample_weight=None):
    return _get_hip().dense_eval_from_margins_packed(
        pk, margins, labels, loss_type, mask, need_grad, sample_weight)


def dense_grad_from_mult_packed(pk, mult: torch.Tensor) -> torch.Tensor:
    return _get_hip().dense_grad_from_mult_packed(pk, mult)


def dense_pack_decode(pk, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 [n, d] from a packed copy, bit for bit: the HIP decoder on the
    GPU, ``packing.decode_torch`` elsewhere."""
    if _use_hip(pk.packed):
        return _get_hip().dense_pack_decode(pk, out)
    from ..packing import decode_torch

    dec = decode_torch(pk.packed, pk.table, pk.d, pk.esc)
    return dec if out is None else out.copy_(dec)


def dense_margins(features: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    if _use_hip(features):
        return _get_hip().dense_margins(features, v)
    return reference.dense_margins(features, v)


def dense_eval_from_margins(features, margins, labels, loss_type, mask=None,
                            need_grad=True, sample_weight=None):
    if _use_hip(features):
        return _get_hip().dense_eval_from_margins(features, margins, labels,
                                                  loss_type, mask, need_grad,
                                                  sample_weight)
    return reference.dense_eval_from_margins(features, margins, labels,
                                             loss_type, mask, need_grad,
                                             sample_weight)


def dense_multiplier_loss(features, margins, labels, loss_type, mask=None,
                          sample_weight=None):
    if _use_hip(features):
        return _get_hip().dense_multiplier_loss(features, margins, labels,
                                                loss_type, mask, sample_weight)
    return reference.dense_multiplier_loss(features, margins, labels,
                                           loss_type, mask, sample_weight)


def dense_grad_from_mult(features, mult):
    if _use_hip(features):
        return _get_hip().dense_grad_from_mult(features, mult)
    return reference.dense_grad_from_mult(features, mult)


def csr_margins(rowptr, col, val, v):
    if _use_hip(val):
        return _get_hip().csr_margins(rowptr, col, val, v)
    return reference.csr_margins(rowptr, col, val, v)


def csr_eval_from_margins(rowptr, col, val, margins, labels, loss_type,
                          mask=None, d=None, csc=None, need_grad=True,
                          sample_weight=None, csc_heavy=None):
    if _use_hip(val):
        return _get_hip().csr_eval_from_margins(rowptr, col, val, margins, labels,
                                                loss_type, mask, d, csc,
                                                need_grad, sample_weight,
                                                csc_heavy)
    return reference.csr_eval_from_margins(rowptr, col, val, margins, labels,
                                           loss_type, mask, d, csc, need_grad,
                                           sample_weight)


def at_margin_update(zm_old, xm_old, gm, pz: float, pg: float, theta: float,
                     offset=None):
    """Fused AT margin update: zm' = pz*zm + pg*gm; xm' = (1-th)*xm + th*zm'
    — one pass on GPU, the axpby composition on CPU (identical algebra).

    ``offset=(coef, src, idx)`` adds the constant ``coef * src[idx]`` to every
    zm' (the margin correction of an unpenalised intercept, read from the
    device vector ``src``); ``None`` is the plain update."""
    if offset is None:
        if _use_hip(zm_old):
            return _get_hip().at_margin_update(zm_old, xm_old, gm, pz, pg, theta)
        zm_new = pz * zm_old + pg * gm
        xm_new = (1.0 - theta) * xm_old + theta * zm_new
        return zm_new, xm_new
    coef, src, idx = offset
    if _use_hip(zm_old):
        return _get_hip().at_margin_update_off(zm_old, xm_old, gm, pz, pg,
                                               theta, coef, src, idx)
    zm_new = pz * zm_old + pg * gm + coef * src[idx].to(zm_old.dtype)
    xm_new = (1.0 - theta) * xm_old + theta * zm_new
    return zm_new, xm_new


def prox(
    kind: int, w: torch.Tensor, g: torch.Tensor, step: float, lam: float,
    lam2: float = 0.0, n_free: int = 0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """One proximal step + regularisation value. The last ``n_free``
    coordinates (an unpenalised intercept) take the plain gradient step and
    stay out of the regularisation value."""
    if n_free == 0:
        if _use_hip(w):
            return _get_hip().prox(kind, w, g, step, lam, lam2)
        return reference.prox(kind, w, g, step, lam, lam2)
    if _use_hip(w):
        return _get_hip().prox_free(kind, w, g, step, lam, lam2, n_free)
    return reference.prox_free(kind, w, g, step, lam, lam2, n_free)


def multiplier_loss_sum(margins, labels, loss_type, mask=None,
                        sample_weight=None):
    """(mult [n], f64[3] = {loss, count, Σmult}) from margins."""
    if _use_hip(margins):
        return _get_hip().multiplier_loss_sum(margins, labels, loss_type,
                                              mask, sample_weight)
    return reference.multiplier_loss_sum(margins, labels, loss_type, mask,
                                         sample_weight)


def add_bias_(margins: torch.Tensor, coef: float, src: torch.Tensor,
              idx: int) -> torch.Tensor:
    """In place ``margins += coef * src[idx]`` with ``src`` a vector on the
    margins' device: the bias is never fetched to the host."""
    if _use_hip(margins):
        return _get_hip().add_bias_(margins, coef, src, idx)
    return reference.add_bias_(margins, coef, src, idx)


def csr_grad_from_mult(rowptr, col, val, mult, d: int, csc=None,
                       csc_heavy=None) -> torch.Tensor:
    """A^T @ mult for a CSR shard from a caller-supplied multiplier."""
    if _use_hip(val):
        return _get_hip().csr_grad_from_mult(rowptr, col, val, mult, d, csc,
                                             csc_heavy)
    return reference.csr_grad_from_mult(rowptr, col, val, mult, d)


def axpby(
    a: float, x: torch.Tensor, b: float, y: torch.Tensor, out: Optional[torch.Tensor] = None
) -> torch.Tensor:
    if _use_hip(x):
        return _get_hip().axpby(a, x, b, y, out)
    return reference.axpby(a, x, b, y, out)


def fused_scalars(
    x: torch.Tensor, y: torch.Tensor, g_y: torch.Tensor, x_old: torch.Tensor
) -> torch.Tensor:
    if _use_hip(x):
        return _get_hip().fused_scalars(x, y, g_y, x_old)
    return reference.fused_scalars(x, y, g_y, x_old)


def dot_diff(
    x: torch.Tensor, y: torch.Tensor, g_x: torch.Tensor, g_y: torch.Tensor
) -> torch.Tensor:
    if _use_hip(x):
        return _get_hip().dot_diff(x, y, g_x, g_y)
    return reference.dot_diff(x, y, g_x, g_y)


def dense_colstats(features: torch.Tensor):
    """Per-column (sum f64, sumsq f64, min f32, max f32, nnz i64), each [d]."""
    if _use_hip(features):
        return _get_hip().dense_colstats(features)
    return reference.dense_colstats(features)


def csr_colstats(csc, n: int, d: int, csc_heavy=None):
    """The dense_colstats tuple over the stored entries of a CSC copy
    ``(colptr, row, val)``; implicit zeros are the caller's to fold in."""
    if _use_hip(csc[2]):
        return _get_hip().csr_colstats(csc, n, d, csc_heavy)
    return reference.csr_colstats(csc, n, d, csc_heavy)


def dense_scale_cols(features: torch.Tensor, scale: torch.Tensor,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if _use_hip(features):
        return _get_hip().dense_scale_cols(features, scale, out)
    return reference.dense_scale_cols(features, scale, out)


def csr_scale_vals(col: torch.Tensor, val: torch.Tensor, scale: torch.Tensor,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if _use_hip(val):
        return _get_hip().csr_scale_vals(col, val, scale, out)
    return reference.csr_scale_vals(col, val, scale, out)


def csc_scale_vals(colptr: torch.Tensor, val: torch.Tensor, scale: torch.Tensor,
                   out: Optional[torch.Tensor] = None, csc_heavy=None) -> torch.Tensor:
    if _use_hip(val):
        return _get_hip().csc_scale_vals(colptr, val, scale, out, csc_heavy)
    return reference.csc_scale_vals(colptr, val, scale, out, csc_heavy)


def binary_metrics(margins: torch.Tensor, labels: torch.Tensor,
                   edges: torch.Tensor, cut: float,
                   sample_weight: Optional[torch.Tensor] = None):
    """One fused pass from margins / labels / weights to (hist_pos i64[B],
    hist_neg i64[B], conf i64[4], sums f64[7], nan_count, min_weight); the
    contract is spelled out on ``reference.binary_metrics``."""
    if _use_hip(margins):
        return _get_hip().binary_metrics(margins, labels, edges, cut,
                                         sample_weight)
    return reference.binary_metrics(margins, labels, edges, cut, sample_weight)


__all__ = [
    "LOSS_LOGISTIC",
    "LOSS_LEAST_SQUARES",
    "LOSS_HINGE",
    "LOSS_SMOOTH_HINGE",
    "PROX_SIMPLE",
    "PROX_L1",
    "PROX_SQUARED_L2",
    "PROX_ELASTIC_NET",
    "dense_eval",
    "csr_eval",
    "dense_margins",
    "dense_multiplier_loss",
    "dense_grad_from_mult",
    "dense_eval_from_margins",
    "csr_margins",
    "csr_eval_from_margins",
    "csr_grad_from_mult",
    "multiplier_loss_sum",
    "add_bias_",
    "at_margin_update",
    "prox",
    "axpby",
    "fused_scalars",
    "dot_diff",
    "dense_colstats",
    "csr_colstats",
    "dense_scale_cols",
    "csr_scale_vals",
    "csc_scale_vals",
    "binary_metrics",
    "hip_available",
    "reference",
]
