"""Column statistics and feature standardisation.

MLlib's ``Statistics.colStats`` and the ``StandardScaler(withStd = true,
withMean = false)`` that every MLlib GLM trainer runs over the features before
optimising (``GeneralizedLinearAlgorithm.useFeatureScaling``), rebuilt for
device-resident shards: one streaming pass of HIP column-moment kernels per
shard, one all-reduce of the moments across ranks, and one in-place (or
out-of-place) column-scaling pass.

AGD's iteration count follows the conditioning of ``A^T A``; dividing each
column by its standard deviation is the cheapest fix for columns whose scales
differ by orders of magnitude.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Union

import torch

from . import ops
from .data import CSRShard, DenseShard, MixedShard
from .parallel.comm import Communicator
from .streaming import HostStreamedDenseShard


@dataclass
class ColumnSummary:
    """Per-column statistics of a (possibly multi-rank) design matrix.

    ``count`` is the global number of rows. ``mean``, ``variance`` (unbiased,
    denominator ``count - 1``; 0 when ``count <= 1``), ``std`` and ``norm_l2``
    are f64 ``[d]`` tensors on the shard's device; ``min`` / ``max`` are f32
    ``[d]``; ``num_nonzeros`` is int64 ``[d]``.
    """

    count: int
    mean: torch.Tensor
    variance: torch.Tensor
    std: torch.Tensor
    num_nonzeros: torch.Tensor
    min: torch.Tensor
    max: torch.Tensor
    norm_l2: torch.Tensor


def _dense_moments(features: torch.Tensor):
    d = features.shape[1]
    if features.shape[0] == 0:
        dev = features.device
        inf = torch.full((d,), float("inf"), dtype=torch.float32, device=dev)
        return (torch.zeros(d, dtype=torch.float64, device=dev),
                torch.zeros(d, dtype=torch.float64, device=dev), inf, -inf,
                torch.zeros(d, dtype=torch.int64, device=dev))
    return ops.dense_colstats(features)


def _merge(a, b):
    """Combine two moment tuples over disjoint row sets."""
    if a is None:
        return b
    return (a[0] + b[0], a[1] + b[1], torch.minimum(a[2], b[2]),
            torch.maximum(a[3], b[3]), a[4] + b[4])


def _csr_moments(shard: CSRShard):
    csc, heavy = shard.csc, shard.csc_heavy
    if csc is None:
        # deterministic=False shards carry no CSC copy: build a temporary one
        # (an argsort over the non-zeros, one-time preprocessing cost)
        csc = shard._build_csc()
        heavy = shard._build_csc_heavy(csc)
    s, q, mn, mx, nnz = ops.csr_colstats(csc, shard.n, shard.d, heavy)
    # min / max so far cover stored entries only: a column storing fewer than
    # n entries also holds implicit zeros
    stored = torch.diff(csc[0].to(torch.int64))
    has_zero = stored < shard.n
    zero = torch.zeros_like(mn)
    mn = torch.where(has_zero, torch.minimum(mn, zero), mn)
    mx = torch.where(has_zero, torch.maximum(mx, zero), mx)
    return s, q, mn, mx, nnz


def _local_moments(shard):
    """(sum f64, sumsq f64, min f32, max f32, nnz i64) over this rank's rows."""
    if isinstance(shard, MixedShard):
        acc = None
        for p in shard.parts:
            acc = _merge(acc, _local_moments(p))
        return acc
    if isinstance(shard, HostStreamedDenseShard):
        acc = None

        def step(buf, lo, hi):
            nonlocal acc
            acc = _merge(acc, _dense_moments(buf))

        shard._for_each_chunk(step)
        if acc is None:
            acc = _dense_moments(torch.empty(
                (0, shard.d), dtype=shard.feature_dtype, device=shard.device))
        return acc
    if isinstance(shard, CSRShard):
        return _csr_moments(shard)
    if isinstance(shard, DenseShard):
        return _dense_moments(shard.features)
    raise TypeError(f"column_stats: unsupported shard type {type(shard).__name__}")


def column_stats(shard, comm: Optional[Communicator] = None) -> ColumnSummary:
    """Per-column mean, variance, non-zero count, min, max and L2 norm of the
    design matrix (``Statistics.colStats``).

    Works on ``DenseShard`` (bf16 / f32 / f64 / fp8), ``CSRShard``,
    ``MixedShard`` and ``HostStreamedDenseShard`` (per-chunk moments through
    its chunk loop). On GPU shards the data pass is the HIP column-moment
    kernels: f64 sums from the first element, no atomics, bitwise
    reproducible. Implicit zeros of sparse rows count as samples, as in
    MLlib's summariser.

    The statistics are UNWEIGHTED: ``sample_weight`` does not enter them.

    A ``CSRShard`` built with ``deterministic=False`` has no CSC copy; a
    temporary one is built here (an argsort over the non-zeros) and dropped —
    a one-time preprocessing cost.

    With ``comm.world_size > 1`` the moments are all-reduced in f64 (sum for
    the sums and counts, min / max for the extrema), so every rank derives
    byte-identical statistics from identical reduced inputs.
    """
    s, q, mn, mx, nnz = _local_moments(shard)
    count = int(shard.n)
    if comm is not None and comm.world_size > 1:
        d = s.numel()
        sums = torch.cat([s, q, nnz.to(torch.float64),
                          torch.tensor([float(count)], dtype=torch.float64,
                                       device=s.device)])
        comm.allreduce_(sums)
        s, q = sums[:d].clone(), sums[d:2 * d].clone()
        nnz = sums[2 * d:3 * d].round().to(torch.int64)
        count = int(round(float(sums[3 * d])))
        mn = comm.allreduce_(mn.to(torch.float64), op="min").to(torch.float32)
        mx = comm.allreduce_(mx.to(torch.float64), op="max").to(torch.float32)
    if count > 0:
        mean = s / count
    else:
        mean = torch.zeros_like(s)
    if count > 1:
        var = ((q - s * s / count) / (count - 1)).clamp_(min=0.0)
        # an exactly constant column has variance 0; the two-sum formula can
        # leave a rounding residue there, which 1/std would blow up
        var = torch.where(mn == mx, torch.zeros_like(var), var)
    else:
        var = torch.zeros_like(s)
    return ColumnSummary(count=count, mean=mean, variance=var, std=var.sqrt(),
                         num_nonzeros=nnz, min=mn, max=mx, norm_l2=q.sqrt())


def _scale_dtype(shard) -> torch.dtype:
    """f64 factors for f64 data, f32 otherwise."""
    if isinstance(shard, MixedShard):
        dts = {_scale_dtype(p) for p in shard.parts}
        return torch.float64 if dts == {torch.float64} else torch.float32
    if isinstance(shard, HostStreamedDenseShard):
        dtype = shard.feature_dtype  # features_host may be released
    elif isinstance(shard, CSRShard):
        dtype = shard.val.dtype
    else:
        dtype = shard.features.dtype
    return torch.float64 if dtype == torch.float64 else torch.float32


class StandardScaler:
    """Scale every feature column to unit standard deviation, without
    centring — MLlib's ``StandardScaler(withStd = true, withMean = false)``.
    Centring is left out for MLlib's reason: it would densify sparse data.

    ``fit`` stores the :class:`ColumnSummary` and ``scale`` ``[d]``:
    ``1 / std`` where the variance is positive and ``1.0`` where it is zero.
    The latter is a deliberate departure from MLlib, which zeroes constant
    columns: it lets the all-ones column of :func:`add_intercept` survive
    scaling. ``scale`` is f32 (the precision the kernels multiply in); a shard
    whose data is f64 gets f64 factors so the f64 path stays exact.

    ``with_std=False`` makes every factor 1 (the transform is then a copy).
    """

    def __init__(self, with_std: bool = True):
        self.with_std = bool(with_std)
        self.summary: Optional[ColumnSummary] = None
        self.scale: Optional[torch.Tensor] = None

    def fit(self, shard, comm: Optional[Communicator] = None) -> "StandardScaler":
        self.summary = column_stats(shard, comm)
        var = self.summary.variance
        if self.with_std:
            safe = torch.where(var > 0, self.summary.std, torch.ones_like(var))
            scale = torch.where(var > 0, 1.0 / safe, torch.ones_like(var))
        else:
            scale = torch.ones_like(var)
        self.scale = scale.to(_scale_dtype(shard))
        return self

    def _check_fitted(self, d: int) -> None:
        if self.scale is None:
            raise RuntimeError("StandardScaler.fit must be called first")
        if self.scale.numel() != d:
            raise ValueError(
                f"scaler was fitted on d={self.scale.numel()}, got d={d}")

    def transform(self, shard, inplace: bool = False):
        """Shard of the same kind and dtype with column c multiplied by
        ``scale[c]``.

        ``inplace=True`` overwrites the features (for CSR: ``val`` and the CSC
        ``val``) and returns the same object. Out of place, a dense result
        holds a second copy of the features; a CSR result shares the whole
        sparsity structure (rowptr, col, labels, colptr, CSC rows, heavy-task
        split) with the source and owns only its two value arrays.

        fp8 shards and ``HostStreamedDenseShard`` raise ``NotImplementedError``.
        """
        self._check_fitted(shard.d)
        if isinstance(shard, MixedShard):
            parts = [self.transform(p, inplace) for p in shard.parts]
            return shard if inplace else MixedShard(parts)
        if isinstance(shard, HostStreamedDenseShard):
            raise NotImplementedError(
                "StandardScaler.transform does not support host-streamed "
                "shards: scale the host data before building the shard")
        if isinstance(shard, CSRShard):
            scale = self.scale.to(shard.device)
            val = ops.csr_scale_vals(shard.col, shard.val, scale,
                                     out=shard.val if inplace else None)
            csc_val = None
            if shard.csc is not None:
                csc_val = ops.csc_scale_vals(
                    shard.csc[0], shard.csc[2], scale,
                    out=shard.csc[2] if inplace else None,
                    csc_heavy=shard.csc_heavy)
            if inplace:
                return shard
            return CSRShard._from_parts(shard, val, csc_val)
        if isinstance(shard, DenseShard):
            if shard.features.dtype == torch.float8_e4m3fn:
                raise NotImplementedError(
                    "StandardScaler.transform does not support fp8 shards: "
                    "scale the bf16/f32 features first, then quantise")
            scale = self.scale.to(shard.device)
            out = ops.dense_scale_cols(shard.features, scale,
                                       out=shard.features if inplace else None)
            if inplace:
                shard.unpack()  # a packed copy would hold the unscaled values
                return shard
            return DenseShard(out, shard.labels, shard.sample_weight)
        raise TypeError(f"transform: unsupported shard type {type(shard).__name__}")

    def _col_factor(self, w: torch.Tensor, num_classes: int) -> torch.Tensor:
        d = self.scale.numel()
        if w.numel() != d * num_classes:
            raise ValueError(f"weights must have {d * num_classes} entries")
        return self.scale.to(device=w.device, dtype=w.dtype)

    def unscale_weights(self, w: torch.Tensor, num_classes: int = 1) -> torch.Tensor:
        """Weights trained on the transformed shard, mapped back to the
        original feature space (``w * scale``; feature-major ``[d, K]`` for
        multiclass), so that ``margins(original, unscale_weights(w)) ==
        margins(transformed, w)``."""
        self._check_fitted(self.scale.numel())
        s = self._col_factor(w, num_classes)
        if num_classes == 1:
            return w * s
        return (w.reshape(-1, num_classes) * s[:, None]).reshape(-1)

    def scale_weights(self, w: torch.Tensor, num_classes: int = 1) -> torch.Tensor:
        """Inverse of :meth:`unscale_weights`: original-space weights (e.g. a
        warm start) mapped into the scaled space (``w / scale``)."""
        self._check_fitted(self.scale.numel())
        s = self._col_factor(w, num_classes)
        if num_classes == 1:
            return w / s
        return (w.reshape(-1, num_classes) / s[:, None]).reshape(-1)


def scaled_training_data(data, feature_scaling: Union[bool, str],
                         comm: Optional[Communicator],
                         initial_weights: Optional[torch.Tensor],
                         num_classes: int = 1):
    """Trainer helper: ``(data, scaler, initial_weights)`` for a
    ``feature_scaling`` option of ``False`` (untouched, scaler ``None``),
    ``True`` (fit + out-of-place transform) or ``"inplace"`` (fit + overwrite
    the caller's shard). ``initial_weights`` are taken to be in the original
    feature space and mapped into the scaled one."""
    if feature_scaling is False or feature_scaling is None:
        return data, None, initial_weights
    if feature_scaling is not True and feature_scaling != "inplace":
        raise ValueError(
            f"feature_scaling must be False, True or 'inplace', got {feature_scaling!r}")
    scaler = StandardScaler().fit(data, comm)
    data = scaler.transform(data, inplace=(feature_scaling == "inplace"))
    if initial_weights is not None:
        initial_weights = scaler.scale_weights(initial_weights, num_classes)
    return data, scaler, initial_weights


__all__ = ["ColumnSummary", "column_stats", "StandardScaler"]
