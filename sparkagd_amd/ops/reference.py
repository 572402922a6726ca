"""Plain-PyTorch reference implementations of every compute primitive.

These are the *oracles*: the CPU execution path for tests/CI (this container has
no GPU) and the ground truth every HIP kernel is validated against
(``tests/test_gpu_kernels.py``). They intentionally use nothing but dense torch
ops, mirroring the role Breeze/netlib BLAS plays under the reference
(``AcceleratedGradientDescent.scala:23,196-207``) and the per-example
``Gradient.compute`` semantics of MLlib 1.3 (usage site ``AGD.scala:198``).

Loss/multiplier conventions (z = <w, x_i> is the *dot product*, NOT MLlib's
negated "margin"; algebra normalized so all three losses share one structure):

  logistic     : mult = sigmoid(z) - y            loss = y>0 ? softplus(-z) : softplus(z)
  least squares: mult = 2 (z - y)                 loss = (z - y)^2
  hinge        : s = 2y - 1
                 mult = (s*z < 1) ? -s : 0        loss = max(0, 1 - s*z)

  grad_sum = A^T mult ; loss_sum = sum loss ; count = #rows (masked rows excluded)

These are algebraically identical to MLlib 1.3's LogisticGradient /
LeastSquaresGradient / HingeGradient (margin = -z substitution).
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

LOSS_LOGISTIC = 0
LOSS_LEAST_SQUARES = 1
LOSS_HINGE = 2
LOSS_SMOOTH_HINGE = 3

PROX_SIMPLE = 0
PROX_L1 = 1
PROX_SQUARED_L2 = 2
PROX_ELASTIC_NET = 3


def _multiplier_and_loss(
    z: torch.Tensor, labels: torch.Tensor, loss_type: int
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Elementwise multiplier m_i and per-example loss l_i from dots z_i."""
    z = z.to(torch.float32) if z.dtype == torch.bfloat16 else z
    y = labels.to(z.dtype)
    if loss_type == LOSS_LOGISTIC:
        mult = torch.sigmoid(z) - y
        loss = torch.where(y > 0, torch.nn.functional.softplus(-z), torch.nn.functional.softplus(z))
    elif loss_type == LOSS_LEAST_SQUARES:
        diff = z - y
        mult = 2.0 * diff
        loss = diff * diff
    elif loss_type == LOSS_HINGE:
        s = 2.0 * y - 1.0
        viol = s * z < 1.0
        mult = torch.where(viol, -s, torch.zeros_like(z))
        loss = torch.clamp(1.0 - s * z, min=0.0)
    elif loss_type == LOSS_SMOOTH_HINGE:
        # Rennie's quadratically smoothed hinge: differentiable, so the
        # accelerated method's smoothness assumptions hold (plain hinge is
        # nonsmooth and is kept for MLlib parity).
        s = 2.0 * y - 1.0
        sz = s * z
        mult = torch.where(sz >= 1.0, torch.zeros_like(z),
                           torch.where(sz > 0.0, -s * (1.0 - sz), -s))
        loss = torch.where(sz >= 1.0, torch.zeros_like(z),
                           torch.where(sz > 0.0, 0.5 * (1.0 - sz) ** 2, 0.5 - sz))
    else:
        raise ValueError(f"unknown loss_type {loss_type}")
    return mult, loss


def _apply_mask_weight(mult, loss, mask, sample_weight, n, device):
    """Apply the mini-batch mask and/or per-example weights; count is the
    number of unmasked examples (sum of their weights when weighted)."""
    if mask is not None:
        m = mask.to(mult.dtype)
        mult = mult * m
        loss = loss * m
    if sample_weight is not None:
        sw = sample_weight.to(mult.dtype)
        mult = mult * sw
        loss = loss * sw
        if mask is not None:
            count = (mask.to(torch.float64) * sample_weight.to(torch.float64)).sum()
        else:
            count = sample_weight.to(torch.float64).sum()
    elif mask is not None:
        count = mask.sum().to(torch.float64)
    else:
        count = torch.tensor(float(n), dtype=torch.float64, device=device)
    return mult, loss, count


def dense_eval(
    features: torch.Tensor,
    labels: torch.Tensor,
    w: torch.Tensor,
    loss_type: int,
    mask: Optional[torch.Tensor] = None,
    need_grad: bool = True,
    sample_weight: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Batched loss/gradient over a dense shard.

    Equivalent of one partition's seqOp fold in the reference's
    ``applySmooth`` (``AGD.scala:196-200``), batched: one GEMV pair instead of
    n per-example axpy/dot calls.

    Returns ``(grad_sum, loss_count)`` where grad_sum has w's dtype and shape
    [d], and loss_count is float64 [2] = (sum of losses, number of examples).
    """
    acc_dtype = torch.float32 if features.dtype in (torch.bfloat16, torch.float16, torch.float8_e4m3fn) else features.dtype
    wa = w.to(acc_dtype)
    z = (features.to(acc_dtype) @ wa) if features.dtype in (torch.bfloat16, torch.float16, torch.float8_e4m3fn) else (features @ wa)
    mult, loss = _multiplier_and_loss(z, labels, loss_type)
    mult, loss, count = _apply_mask_weight(mult, loss, mask, sample_weight,
                                           features.shape[0], features.device)
    loss_count = torch.stack([loss.to(torch.float64).sum(), count])
    if not need_grad:
        return None, loss_count
    grad_sum = (features.to(acc_dtype).T @ mult.to(acc_dtype)).to(w.dtype)
    return grad_sum, loss_count


def csr_eval(
    rowptr: torch.Tensor,
    col: torch.Tensor,
    val: torch.Tensor,
    labels: torch.Tensor,
    w: torch.Tensor,
    loss_type: int,
    mask: Optional[torch.Tensor] = None,
    d: Optional[int] = None,
    need_grad: bool = True,
    sample_weight: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Batched loss/gradient over a CSR shard (MLlib sparse-Vector path analog)."""
    n = rowptr.numel() - 1
    d = d if d is not None else w.numel()
    acc_dtype = torch.float32 if val.dtype in (torch.bfloat16, torch.float16) else val.dtype
    a = torch.sparse_csr_tensor(
        rowptr.to(torch.int64), col.to(torch.int64), val.to(acc_dtype), size=(n, d)
    )
    z = a @ w.to(acc_dtype)
    mult, loss = _multiplier_and_loss(z, labels, loss_type)
    mult, loss, count = _apply_mask_weight(mult, loss, mask, sample_weight, n, val.device)
    loss_count = torch.stack([loss.to(torch.float64).sum(), count])
    if not need_grad:
        return None, loss_count
    grad_sum = (a.t() @ mult.to(acc_dtype)).to(w.dtype)
    return grad_sum, loss_count


def dense_margins(features: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """margins = A @ v (margin-state tracking support)."""
    acc = torch.float32 if features.dtype in (torch.bfloat16, torch.float16, torch.float8_e4m3fn) else features.dtype
    return features.to(acc) @ v.to(acc)


def dense_eval_from_margins(
    features: torch.Tensor,
    margins: torch.Tensor,
    labels: torch.Tensor,
    loss_type: int,
    mask: Optional[torch.Tensor] = None,
    need_grad: bool = True,
    sample_weight: Optional[torch.Tensor] = None,
) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    acc = torch.float32 if features.dtype in (torch.bfloat16, torch.float16, torch.float8_e4m3fn) else features.dtype
    mult, loss = _multiplier_and_loss(margins, labels, loss_type)
    mult, loss, count = _apply_mask_weight(mult, loss, mask, sample_weight,
                                           features.shape[0], features.device)
    loss_count = torch.stack([loss.to(torch.float64).sum(), count])
    if not need_grad:
        return None, loss_count
    grad_sum = (features.to(acc).T @ mult.to(acc))
    return grad_sum, loss_count


def dense_multiplier_loss(
    features: torch.Tensor,
    margins: torch.Tensor,
    labels: torch.Tensor,
    loss_type: int,
    mask: Optional[torch.Tensor] = None,
    sample_weight: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    mult, loss = _multiplier_and_loss(margins, labels, loss_type)
    mult, loss, count = _apply_mask_weight(mult, loss, mask, sample_weight,
                                           features.shape[0], features.device)
    return mult, torch.stack([loss.to(torch.float64).sum(), count])


def dense_grad_from_mult(features: torch.Tensor, mult: torch.Tensor) -> torch.Tensor:
    acc = torch.float32 if features.dtype in (torch.bfloat16, torch.float16, torch.float8_e4m3fn) else features.dtype
    return features.to(acc).T @ mult.to(acc)


def csr_margins(rowptr, col, val, v: torch.Tensor, n: Optional[int] = None) -> torch.Tensor:
    n = rowptr.numel() - 1
    # f64 values keep f64 margins (as csr_eval does); everything narrower
    # accumulates in f32 like the kernels
    acc = torch.float64 if val.dtype == torch.float64 else torch.float32
    a = torch.sparse_csr_tensor(rowptr.to(torch.int64), col.to(torch.int64),
                                val.to(acc), size=(n, v.numel()))
    return a @ v.to(acc)


def csr_eval_from_margins(rowptr, col, val, margins, labels, loss_type,
                          mask=None, d=None, csc=None, need_grad=True,
                          sample_weight=None):
    n = rowptr.numel() - 1
    mult, loss = _multiplier_and_loss(margins, labels, loss_type)
    mult, loss, count = _apply_mask_weight(mult, loss, mask, sample_weight, n, val.device)
    loss_count = torch.stack([loss.to(torch.float64).sum(), count])
    if not need_grad:
        return None, loss_count
    a = torch.sparse_csr_tensor(rowptr.to(torch.int64), col.to(torch.int64),
                                val.to(torch.float32), size=(n, d))
    grad_sum = a.t() @ mult.to(torch.float32)
    return grad_sum, loss_count


def prox(
    kind: int,
    w: torch.Tensor,
    g: torch.Tensor,
    step: float,
    lam: float,
    lam2: float = 0.0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """One proximal-gradient step + regularization value.

    Semantics of MLlib 1.3's SimpleUpdater / L1Updater / SquaredL2Updater
    (invoked by the reference at ``AGD.scala:215-220``), with the
    stepSize/sqrt(iter) internal rescaling handled by the *caller*
    (models/updater.py), since AGD always passes iter=1 exactly to defeat it.

    Returns ``(w_new, reg_value)`` with reg_value a float64 scalar tensor.
    """
    if kind == PROX_SIMPLE:
        w_new = w - step * g
        reg = torch.zeros((), dtype=torch.float64, device=w.device)
    elif kind == PROX_L1:
        w1 = w - step * g
        shrink = lam * step
        w_new = torch.sign(w1) * torch.clamp(w1.abs() - shrink, min=0.0)
        reg = lam * w_new.abs().to(torch.float64).sum()
    elif kind == PROX_SQUARED_L2:
        w_new = w * (1.0 - step * lam) - step * g
        reg = 0.5 * lam * (w_new.to(torch.float64) ** 2).sum()
    elif kind == PROX_ELASTIC_NET:
        # prox of lam*|w|_1 + lam2/2*|w|^2: soft-threshold then shrink
        w1 = w - step * g
        wsoft = torch.sign(w1) * torch.clamp(w1.abs() - lam * step, min=0.0)
        w_new = wsoft / (1.0 + step * lam2)
        reg = (lam * w_new.abs().to(torch.float64).sum()
               + 0.5 * lam2 * (w_new.to(torch.float64) ** 2).sum())
    else:
        raise ValueError(f"unknown prox kind {kind}")
    return w_new, reg


def prox_free(kind: int, w: torch.Tensor, g: torch.Tensor, step: float,
              lam: float, lam2: float, n_free: int
              ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``prox`` whose last ``n_free`` coordinates take the plain step
    ``w - step*g`` whatever ``kind`` is and add nothing to the regularisation
    value (an unpenalised intercept stored last)."""
    n = w.numel()
    if not 0 <= n_free <= n:
        raise ValueError(f"n_free {n_free} outside [0, {n}]")
    k = n - n_free
    head, reg = prox(kind, w[:k], g[:k], step, lam, lam2)
    return torch.cat([head, w[k:] - step * g[k:]]), reg


def multiplier_loss_sum(
    margins: torch.Tensor,
    labels: torch.Tensor,
    loss_type: int,
    mask: Optional[torch.Tensor] = None,
    sample_weight: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mult [n], f64[3] = {loss sum, count, sum of mult}) from margins; the
    third entry is the gradient of an intercept (masked rows count 0,
    weighted rows m*sw)."""
    mult, loss = _multiplier_and_loss(margins, labels, loss_type)
    mult, loss, count = _apply_mask_weight(mult, loss, mask, sample_weight,
                                           margins.numel(), margins.device)
    return mult, torch.stack([loss.to(torch.float64).sum(), count,
                              mult.to(torch.float64).sum()])


def add_bias_(margins: torch.Tensor, coef: float, src: torch.Tensor,
              idx: int) -> torch.Tensor:
    """In place margins += coef * src[idx]."""
    margins.add_(src[idx].to(margins.dtype), alpha=coef)
    return margins


def csr_grad_from_mult(rowptr, col, val, mult: torch.Tensor, d: int
                       ) -> torch.Tensor:
    """A^T @ mult over a CSR shard (f64 for f64 values, else f32)."""
    n = rowptr.numel() - 1
    acc = torch.float64 if val.dtype == torch.float64 else torch.float32
    a = torch.sparse_csr_tensor(rowptr.to(torch.int64), col.to(torch.int64),
                                val.to(acc), size=(n, d))
    return a.t() @ mult.to(acc)


def axpby(a: float, x: torch.Tensor, b: float, y: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = a*x + b*y (the reference's affine combinations, ``AGD.scala:249,255``)."""
    if out is None:
        out = torch.empty_like(x)
    torch.add(a * x, y, alpha=b, out=out)
    return out


def fused_scalars(
    x: torch.Tensor,
    y: torch.Tensor,
    g_y: torch.Tensor,
    x_old: torch.Tensor,
) -> torch.Tensor:
    """One pass producing the 5 iteration scalars as float64 [5]:

      [0] ||x - y||^2          (backtracking xy_sq,      AGD.scala:263-264)
      [1] <x - y, g_y>         (simple backtrack test,   AGD.scala:273)
      [2] ||x||^2              (convergence,             AGD.scala:315)
      [3] ||x - x_old||^2      (convergence,             AGD.scala:316)
      [4] <g_y, x - x_old>     (gradient-test restart,   AGD.scala:327)
    """
    xd = x.to(torch.float64)
    xy = xd - y.to(torch.float64)
    dx = xd - x_old.to(torch.float64)
    gy = g_y.to(torch.float64)
    return torch.stack(
        [
            (xy * xy).sum(),
            (xy * gy).sum(),
            (xd * xd).sum(),
            (dx * dx).sum(),
            (gy * dx).sum(),
        ]
    )


def dot_diff(x: torch.Tensor, y: torch.Tensor, g_x: torch.Tensor, g_y: torch.Tensor) -> torch.Tensor:
    """<x - y, g_x - g_y> as float64 scalar (alternate backtrack test, AGD.scala:278)."""
    xy = x.to(torch.float64) - y.to(torch.float64)
    dg = g_x.to(torch.float64) - g_y.to(torch.float64)
    return (xy * dg).sum()


# ---------------------------------------------------------------------------
# Column statistics / column scaling oracles
# ---------------------------------------------------------------------------

def dense_colstats(features: torch.Tensor):
    """Per-column (sum f64, sumsq f64, min f32, max f32, nnz i64) of a dense
    [n, d] matrix, everything accumulated in f64 (Statistics.colStats
    moments). An empty matrix reports min +inf / max -inf."""
    a = features.to(torch.float64)
    n, d = a.shape
    if n == 0:
        mn = torch.full((d,), float("inf"), dtype=torch.float32, device=a.device)
        mx = -mn
    else:
        mn = a.amin(dim=0).to(torch.float32)
        mx = a.amax(dim=0).to(torch.float32)
    return (a.sum(dim=0), (a * a).sum(dim=0), mn, mx,
            (a != 0).sum(dim=0).to(torch.int64))


def _csc_cols(colptr: torch.Tensor) -> torch.Tensor:
    d = colptr.numel() - 1
    return torch.repeat_interleave(
        torch.arange(d, device=colptr.device, dtype=torch.int64),
        torch.diff(colptr.to(torch.int64)))


def csr_colstats(csc, n: int, d: int, csc_heavy=None):
    """The dense_colstats tuple over the STORED entries of a CSC copy
    (colptr, row, val): empty columns report sum 0, min +inf, max -inf, and
    the caller folds in the implicit zeros."""
    colptr, _row, val = csc
    cols = _csc_cols(colptr)
    v = val.to(torch.float64)
    dev = val.device
    s = torch.zeros(d, dtype=torch.float64, device=dev).index_add_(0, cols, v)
    q = torch.zeros(d, dtype=torch.float64, device=dev).index_add_(0, cols, v * v)
    mn = torch.full((d,), float("inf"), dtype=torch.float64, device=dev)
    mn.scatter_reduce_(0, cols, v, reduce="amin", include_self=True)
    mx = torch.full((d,), float("-inf"), dtype=torch.float64, device=dev)
    mx.scatter_reduce_(0, cols, v, reduce="amax", include_self=True)
    nnz = torch.zeros(d, dtype=torch.int64, device=dev).index_add_(
        0, cols, (v != 0).to(torch.int64))
    return s, q, mn.to(torch.float32), mx.to(torch.float32), nnz


def _scale_acc(dtype: torch.dtype) -> torch.dtype:
    return torch.float64 if dtype == torch.float64 else torch.float32


def dense_scale_cols(features: torch.Tensor, scale: torch.Tensor,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """features * scale[None, :] through one multiply in f32 (f64 for f64
    features), rounded back to the features dtype."""
    if features.dtype == torch.float8_e4m3fn:
        raise NotImplementedError(
            "fp8 features cannot be rescaled in place of their quantisation: "
            "scale the bf16/f32 data first, then quantise")
    acc = _scale_acc(features.dtype)
    res = (features.to(acc) * scale.to(device=features.device, dtype=acc)).to(features.dtype)
    if out is None:
        return res
    out.copy_(res)
    return out


def csr_scale_vals(col: torch.Tensor, val: torch.Tensor, scale: torch.Tensor,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    res = val * scale.to(device=val.device, dtype=val.dtype)[col.to(torch.int64)]
    if out is None:
        return res
    out.copy_(res)
    return out


def csc_scale_vals(colptr: torch.Tensor, val: torch.Tensor, scale: torch.Tensor,
                   out: Optional[torch.Tensor] = None, csc_heavy=None) -> torch.Tensor:
    res = val * scale.to(device=val.device, dtype=val.dtype)[_csc_cols(colptr)]
    if out is None:
        return res
    out.copy_(res)
    return out


# --- evaluation metrics (oracles of k_binary_metrics / k_multiclass_metrics) ---

METRICS_MAX_BINS = 4096
METRICS_FIXED_ONE = 2 ** 32  # a weighted example counts llrint(w * 2^32) units


def stable_softplus(t: torch.Tensor) -> torch.Tensor:
    """log(1 + e^t) as t + log1p(e^-t) for t > 0 and log1p(e^t) otherwise:
    exact to rounding for every t, 0 at -inf and +inf at +inf (the form the
    HIP kernels use; ``torch.nn.functional.softplus`` switches to the
    identity above 20 and so differs by up to 2e-9 there)."""
    return torch.where(t > 0, t + torch.log1p(torch.exp(-t)),
                       torch.log1p(torch.exp(t)))


def _metric_weights(sample_weight: Optional[torch.Tensor], n: int, device):
    """(integer units [n] i64, weights [n] f64, min weight f32 0-dim)."""
    if sample_weight is None:
        return (torch.ones(n, dtype=torch.int64, device=device),
                torch.ones(n, dtype=torch.float64, device=device),
                torch.tensor(float("inf"), dtype=torch.float32, device=device))
    w32 = sample_weight.to(device=device, dtype=torch.float32)
    w = w32.to(torch.float64)
    units = (w * METRICS_FIXED_ONE).round().to(torch.int64)
    wmin = (w32.min() if n > 0 else
            torch.tensor(float("inf"), dtype=torch.float32, device=device))
    return units, w, wmin


def binary_metrics(margins: torch.Tensor, labels: torch.Tensor,
                   edges: torch.Tensor, cut: float,
                   sample_weight: Optional[torch.Tensor] = None):
    """Every sufficient statistic of the binary / regression metrics in one
    pass over ``margins`` [n] (f32 or f64), ``labels`` [n] and optional
    ``sample_weight`` [n] (f32):

    * ``hist_pos``, ``hist_neg`` int64 [B], B = len(edges) + 1: the bin of z
      is the number of edges <= z (``torch.bucketize(right=True)``; ``edges``
      strictly increasing, in the margins' dtype); an example is positive
      when y > 0.5 and adds 1, or ``round(w * 2^32)`` when weighted;
    * ``conf`` int64 [4] = (tp, fp, fn, tn) for the prediction ``z > cut``
      (``cut`` rounded to the margins' dtype), same units;
    * ``sums`` f64 [7] = Σw, Σw·logloss(z, y), Σw·(z−y)², Σw·|z−y|, Σw·y,
      Σw·y², Σw·(z−y), each term evaluated in f64 from the stored margin,
      the log-loss through :func:`stable_softplus`;
    * ``nan_count`` int64 0-dim: NaN margins, which enter nothing else;
    * ``min_weight`` f32 0-dim (+inf when unweighted).
    """
    if margins.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"margins must be f32 or f64, got {margins.dtype}")
    z = margins.reshape(-1)
    n = z.numel()
    dev = z.device
    edges = edges.to(device=dev, dtype=z.dtype).reshape(-1)
    nbins = edges.numel() + 1
    if nbins > METRICS_MAX_BINS:
        raise ValueError(f"at most {METRICS_MAX_BINS} bins, got {nbins}")
    units, w, wmin = _metric_weights(sample_weight, n, dev)
    keep = ~torch.isnan(z)
    nan_count = (~keep).sum().to(torch.int64)
    z, y = z[keep], labels.to(dev).reshape(-1)[keep]
    units, w = units[keep], w[keep]
    pos = y > 0.5
    if nbins > 1:
        bins = torch.bucketize(z, edges, right=True)
    else:
        bins = torch.zeros(z.numel(), dtype=torch.int64, device=dev)
    zero = torch.zeros(nbins, dtype=torch.int64, device=dev)
    hist_pos = zero.clone().index_add_(0, bins[pos], units[pos])
    hist_neg = zero.clone().index_add_(0, bins[~pos], units[~pos])
    pred = z > torch.tensor(cut, dtype=z.dtype, device=dev)
    conf = torch.stack([units[pos & pred].sum(), units[~pos & pred].sum(),
                        units[pos & ~pred].sum(), units[~pos & ~pred].sum()])
    zd, yd = z.to(torch.float64), y.to(torch.float64)
    logloss = torch.where(pos, stable_softplus(-zd), stable_softplus(zd))
    diff = zd - yd
    sums = torch.stack([w.sum(), (w * logloss).sum(), (w * (diff * diff)).sum(),
                        (w * diff.abs()).sum(), (w * yd).sum(),
                        (w * (yd * yd)).sum(), (w * diff).sum()])
    return hist_pos, hist_neg, conf, sums, nan_count, wmin


def argmax_lowest(z: torch.Tensor) -> torch.Tensor:
    """Row argmax of z [n, K] with the LOWEST index winning ties (spelled
    out: ``torch.argmax`` leaves the tie rule unspecified)."""
    k = z.shape[1]
    idx = torch.arange(k, device=z.device).expand_as(z)
    is_max = z == z.max(dim=1, keepdim=True).values
    return torch.where(is_max, idx, torch.full_like(idx, k)).min(dim=1).values


def multiclass_metrics(margins_padded_flat: torch.Tensor, labels: torch.Tensor,
                       k: int, kc: int,
                       sample_weight: Optional[torch.Tensor] = None):
    """Sufficient statistics of the multiclass metrics from padded margins
    [n * kc] (what ``MultinomialLogisticGradient.margins`` returns),
    restricted to the logical ``k`` classes:

    * ``conf`` int64 [k, k], rows = true class, columns = argmax (lowest
      index on ties), in the units of :func:`binary_metrics`;
    * ``sums`` f64 [2] = Σw, Σw·(logsumexp(z) − z_y), the per-row loss
      max-subtracted in the margins' dtype, accumulated in f64;
    * ``bad_labels`` int64 0-dim: labels outside [0, k), left out of ``conf``;
    * ``min_weight`` f32 0-dim (+inf when unweighted).
    """
    n = margins_padded_flat.numel() // kc
    dev = margins_padded_flat.device
    z = margins_padded_flat.reshape(n, kc)[:, :k]
    units, w, wmin = _metric_weights(sample_weight, n, dev)
    y = labels.to(dev).reshape(-1).to(torch.int64)
    valid = (y >= 0) & (y < k)
    bad = (~valid).sum().to(torch.int64)
    pred = argmax_lowest(z)
    yc = y.clamp(0, k - 1)
    zy = torch.where(valid, z.gather(1, yc.unsqueeze(1)).squeeze(1),
                     torch.zeros(n, dtype=z.dtype, device=dev))
    # logsumexp(z) - z_y with the maximum taken out of BOTH terms: a confident
    # correct row (z_y = max) then loses nothing to cancellation in f32
    zmax = z.max(dim=1).values
    loss = torch.log(torch.exp(z - zmax.unsqueeze(1)).sum(dim=1)) + (zmax - zy)
    conf = torch.zeros(k * k, dtype=torch.int64, device=dev).index_add_(
        0, (yc * k + pred)[valid], units[valid]).reshape(k, k)
    sums = torch.stack([w.sum(), (w * loss.to(torch.float64)).sum()])
    return conf, sums, bad, wmin
