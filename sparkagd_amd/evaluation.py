"""Model evaluation metrics (MLlib's BinaryClassificationMetrics /
MulticlassMetrics analog, GPU-resident).

The reference ships no metrics in-repo, but an MLlib 1.3 user evaluates the
trained GLMs with ``mllib.evaluation``; these are the equivalents a user
switching frameworks expects. The functions at the top take plain tensors
(margins / scores / labels) and run on whatever device they live on.

:func:`evaluate` is the shard-native path: it scores a whole shard of any
kind through the shard's own ``margins`` kernels, reduces margins, labels and
sample weights to integer histograms, an integer confusion and a few f64 sums
in ONE fused device pass (``ops.binary_metrics`` /
``ops.multiclass.multiclass_metrics``), all-reduces those across ranks, and
derives every metric on the host in f64 — MLlib's
``BinaryClassificationMetrics(scoreAndLabels, numBins)``,
``MulticlassMetrics`` and ``RegressionMetrics``.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from .ops import reference as _ref


def accuracy(pred: torch.Tensor, labels: torch.Tensor) -> float:
    """Fraction of exact prediction/label matches."""
    return float((pred.to(torch.float32) == labels.to(torch.float32))
                 .to(torch.float64).mean())


def log_loss(margins: torch.Tensor, labels: torch.Tensor) -> float:
    """Mean binary logistic loss from margins z = <w, x> (labels in {0,1})."""
    z = margins.to(torch.float64)
    y = labels.to(torch.float64)
    # log(1+e^-z) for y=1, log(1+e^z) for y=0, computed stably
    return float((torch.nn.functional.softplus(-z) * y
                  + torch.nn.functional.softplus(z) * (1.0 - y)).mean())


def roc_auc(scores: torch.Tensor, labels: torch.Tensor) -> float:
    """Area under the ROC curve via the rank statistic
    AUC = (U - n_pos(n_pos+1)/2) / (n_pos * n_neg), with midrank tie
    handling — equivalent to trapezoidal integration over all thresholds."""
    s = scores.to(torch.float64).flatten()
    y = (labels.to(torch.float64).flatten() > 0.5)
    n_pos = int(y.sum())
    n_neg = y.numel() - n_pos
    if n_pos == 0 or n_neg == 0:
        raise ValueError("roc_auc needs both classes present")
    order = torch.argsort(s)
    sorted_s = s[order]
    ranks = torch.empty_like(s)
    # midranks for ties
    uniq, inv, counts = torch.unique(sorted_s, return_inverse=True,
                                     return_counts=True)
    cum = torch.cumsum(counts.to(torch.float64), 0)
    mid = cum - (counts.to(torch.float64) - 1) / 2.0
    ranks[order] = mid[inv]
    u = float(ranks[y].sum())
    return (u - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg)


def precision_recall_f1(pred: torch.Tensor, labels: torch.Tensor) -> Dict[str, float]:
    """Binary precision/recall/F1 (positive class = 1)."""
    p = pred.to(torch.bool)
    y = labels.to(torch.float32) > 0.5
    tp = float((p & y).sum())
    fp = float((p & ~y).sum())
    fn = float((~p & y).sum())
    prec = tp / (tp + fp) if tp + fp > 0 else 0.0
    rec = tp / (tp + fn) if tp + fn > 0 else 0.0
    f1 = 2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0
    return {"precision": prec, "recall": rec, "f1": f1}


def confusion_matrix(pred: torch.Tensor, labels: torch.Tensor,
                     num_classes: int) -> torch.Tensor:
    """[K, K] counts; rows = true class, cols = predicted."""
    idx = (labels.to(torch.int64) * num_classes + pred.to(torch.int64))
    return torch.bincount(idx, minlength=num_classes * num_classes).reshape(
        num_classes, num_classes)


# ---------------------------------------------------------------------------
# Shard-native evaluation
# ---------------------------------------------------------------------------

MAX_BINS = _ref.METRICS_MAX_BINS
_FIXED_ONE = float(_ref.METRICS_FIXED_ONE)
_MAX_WEIGHT_SUM = float(2 ** 31)


def _ratio(num: float, den: float) -> float:
    return num / den if den > 0 else 0.0


def _f_beta(prec: float, rec: float, beta: float = 1.0) -> float:
    b2 = beta * beta
    return _ratio((1.0 + b2) * prec * rec, b2 * prec + rec)


@dataclass
class BinaryMetrics:
    """Binned binary-classification metrics (``BinaryClassificationMetrics``).

    ``hist_pos`` / ``hist_neg`` [B] are the (weighted) numbers of positive /
    negative examples per margin bin, bin j holding the margins with exactly
    j of the ``edges`` [B-1] at or below them; all counts are f64 in weight
    units (plain counts when the shard has no ``sample_weight``).
    ``confusion`` = (tp, fp, fn, tn) and the four rates are taken at the
    ``threshold`` given to :func:`evaluate`; the curves run over the bin
    edges. ``log_loss`` is ``None`` for a hinge model.
    """

    hist_pos: torch.Tensor
    hist_neg: torch.Tensor
    edges: torch.Tensor
    count: float
    num_positives: float
    num_negatives: float
    confusion: Tuple[float, float, float, float]
    accuracy: float
    precision: float
    recall: float
    f1: float
    log_loss: Optional[float]

    def _cumulative(self):
        """(tp, fp) [B] predicting positive from bin B-1 down to bin j."""
        tp = torch.cumsum(self.hist_pos.flip(0), 0)
        fp = torch.cumsum(self.hist_neg.flip(0), 0)
        return tp, fp

    def roc(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(fpr, tpr) [B+1], from (0, 0) down the thresholds to (1, 1)."""
        tp, fp = self._cumulative()
        zero = torch.zeros(1, dtype=torch.float64)
        return (torch.cat([zero, fp / self.num_negatives]),
                torch.cat([zero, tp / self.num_positives]))

    @property
    def area_under_roc(self) -> float:
        fpr, tpr = self.roc()
        return float(torch.trapezoid(tpr, fpr))

    def pr(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(recall, precision) over the non-empty bins from the top down,
        led by MLlib's first point (0, p1)."""
        tp, fp = self._cumulative()
        seen = (self.hist_pos + self.hist_neg).flip(0) > 0
        tp, fp = tp[seen], fp[seen]
        rec = tp / self.num_positives
        prec = tp / (tp + fp)
        return (torch.cat([torch.zeros(1, dtype=torch.float64), rec]),
                torch.cat([prec[:1], prec]))

    @property
    def area_under_pr(self) -> float:
        rec, prec = self.pr()
        return float(torch.trapezoid(prec, rec))

    def f_measure_by_threshold(self, beta: float = 1.0
                               ) -> Tuple[torch.Tensor, torch.Tensor]:
        """(thresholds, F_beta) [B]: the margin-space lower bound of each bin
        from the top down (-inf for bin 0) and the F-measure of predicting
        positive at or above it (0 where precision and recall are both 0)."""
        tp, fp = self._cumulative()
        thr = torch.cat([torch.full((1,), -math.inf, dtype=torch.float64),
                         self.edges.to(torch.float64)]).flip(0)
        rec = tp / self.num_positives
        prec = torch.where(tp + fp > 0, tp / (tp + fp).clamp(min=1e-300),
                           torch.zeros_like(tp))
        b2 = beta * beta
        den = b2 * prec + rec
        f = torch.where(den > 0, (1.0 + b2) * prec * rec / den.clamp(min=1e-300),
                        torch.zeros_like(den))
        return thr, f


@dataclass
class RegressionMetrics:
    """``RegressionMetrics``: (weighted) mean squared / absolute error, R²
    = 1 − SS_res / SS_tot and explained variance = 1 − Var(y − ŷ) / Var(y)."""

    mse: float
    rmse: float
    mae: float
    r2: float
    explained_variance: float
    count: float


@dataclass
class MulticlassMetrics:
    """``MulticlassMetrics``: ``confusion`` [K, K] f64 in weight units (rows =
    true class, columns = predicted), accuracy, mean softmax ``log_loss``,
    per-class precision / recall / F1 and their averages weighted by the
    true-class frequencies."""

    confusion: torch.Tensor
    accuracy: float
    log_loss: float
    count: float

    def precision(self, k: int) -> float:
        return _ratio(float(self.confusion[k, k]), float(self.confusion[:, k].sum()))

    def recall(self, k: int) -> float:
        return _ratio(float(self.confusion[k, k]), float(self.confusion[k, :].sum()))

    def f1(self, k: int) -> float:
        return _f_beta(self.precision(k), self.recall(k))

    def _weighted(self, fn) -> float:
        total = float(self.confusion.sum())
        return sum(_ratio(float(self.confusion[k].sum()), total) * fn(k)
                   for k in range(self.confusion.shape[0]))

    @property
    def weighted_precision(self) -> float:
        return self._weighted(self.precision)

    @property
    def weighted_recall(self) -> float:
        return self._weighted(self.recall)

    @property
    def weighted_f1(self) -> float:
        return self._weighted(self.f1)


def _edges_for(num_bins: int, thresholds, dtype: torch.dtype) -> torch.Tensor:
    """Margin-space bin edges in the margins' dtype, validated."""
    if thresholds is None:
        if not 1 <= int(num_bins) <= MAX_BINS:
            raise ValueError(f"num_bins must be in [1, {MAX_BINS}], got {num_bins}")
        b = int(num_bins)
        p = torch.arange(1, b, dtype=torch.float64) / b
        e64 = torch.log(p) - torch.log1p(-p)  # logit(j/B): uniform in sigmoid space
    else:
        e64 = torch.as_tensor(thresholds, dtype=torch.float64).reshape(-1).cpu()
        if e64.numel() + 1 > MAX_BINS:
            raise ValueError(f"at most {MAX_BINS - 1} thresholds "
                             f"({MAX_BINS} bins), got {e64.numel()}")
    edges = e64.to(dtype)
    if torch.isnan(edges).any() or not bool((edges[1:] > edges[:-1]).all()):
        raise ValueError(f"thresholds must be strictly increasing in {dtype}")
    return edges


def _reduce(ints: torch.Tensor, sums: torch.Tensor, nan_or_bad: torch.Tensor,
            wmin: torch.Tensor, comm) -> Tuple[torch.Tensor, torch.Tensor, int, bool]:
    """All-reduce one evaluation's integers and f64 sums (one collective
    each) with the two local validity words riding along, so that every rank
    reaches the same verdict; returns host copies."""
    wsum = sums[0]
    bad_w = (~(wmin >= 0)) | ~torch.isfinite(wsum) | (wsum >= _MAX_WEIGHT_SUM)
    ints = torch.cat([ints.reshape(-1), nan_or_bad.reshape(1),
                      bad_w.reshape(1).to(torch.int64)])
    if comm is not None and comm.world_size > 1:
        sums = sums.clone()
        comm.allreduce_(ints)
        comm.allreduce_(sums)
    ints, sums = ints.cpu(), sums.cpu()
    bad_weights = int(ints[-1]) != 0 or not float(sums[0]) < _MAX_WEIGHT_SUM
    return ints[:-2], sums, int(ints[-2]), bad_weights


_WEIGHT_ERROR = ("sample weights must be finite and >= 0 with a total below "
                 "2^31 per rank and overall")


def _binary_stats(z, shard, edges, cut, comm):
    from . import ops

    sw = getattr(shard, "sample_weight", None)
    hp, hn, conf, sums, nan, wmin = ops.binary_metrics(z, shard.labels, edges,
                                                       cut, sw)
    ints, sums, n_nan, bad_w = _reduce(torch.cat([hp, hn, conf]), sums, nan,
                                       wmin, comm)
    if n_nan:
        raise ValueError(f"{n_nan} NaN margins: the model or the data is not finite")
    if bad_w:
        raise ValueError(_WEIGHT_ERROR)
    scale = 1.0 if sw is None else 1.0 / _FIXED_ONE
    b = edges.numel() + 1
    counts = ints.to(torch.float64) * scale
    return counts[:b], counts[b:2 * b], counts[2 * b:], sums.to(torch.float64)


def _evaluate_binary(model, shard, z, comm, num_bins, thresholds, threshold):
    if threshold is None or not 0.0 < float(threshold) < 1.0:
        raise ValueError(f"threshold must be in (0, 1), got {threshold}")
    edges = _edges_for(num_bins, thresholds, z.dtype)
    hp, hn, conf, sums = _binary_stats(z, shard, edges, model._cut(threshold), comm)
    n_pos, n_neg = float(hp.sum()), float(hn.sum())
    if n_pos <= 0 or n_neg <= 0:
        raise ValueError("binary metrics need both classes present")
    tp, fp, fn, tn = (float(c) for c in conf)
    prec, rec = _ratio(tp, tp + fp), _ratio(tp, tp + fn)
    return BinaryMetrics(
        hist_pos=hp, hist_neg=hn, edges=edges, count=n_pos + n_neg,
        num_positives=n_pos, num_negatives=n_neg, confusion=(tp, fp, fn, tn),
        accuracy=_ratio(tp + tn, tp + fp + fn + tn), precision=prec,
        recall=rec, f1=_f_beta(prec, rec),
        log_loss=(float(sums[1] / sums[0]) if model.link == "logistic" else None))


def _evaluate_regression(shard, z, comm):
    edges = torch.empty(0, dtype=z.dtype)
    _, _, _, s = _binary_stats(z, shard, edges, 0.0, comm)
    w, se, ae, sy, syy, sd = (float(s[i]) for i in (0, 2, 3, 4, 5, 6))
    if not w > 0:
        raise ValueError("regression metrics need a positive total weight")
    ss_tot = syy - sy * sy / w
    var_res = se / w - (sd / w) ** 2
    mse = se / w
    return RegressionMetrics(
        mse=mse, rmse=math.sqrt(mse), mae=ae / w,
        r2=1.0 - se / ss_tot if ss_tot > 0 else float("nan"),
        explained_variance=(1.0 - var_res / (ss_tot / w) if ss_tot > 0
                            else float("nan")),
        count=w)


def _evaluate_multiclass(model, shard, zp, comm):
    from .ops import multiclass as mc

    k = model.num_classes
    sw = getattr(shard, "sample_weight", None)
    conf, sums, bad, wmin = mc.multiclass_metrics(zp, shard.labels, k, sw)
    ints, sums, n_bad, bad_w = _reduce(conf, sums, bad, wmin, comm)
    if n_bad:
        raise ValueError(f"{n_bad} labels outside [0, {k})")
    if bad_w:
        raise ValueError(_WEIGHT_ERROR)
    if not bool(torch.isfinite(sums).all()):
        raise ValueError("non-finite margins: the model or the data is not finite")
    scale = 1.0 if sw is None else 1.0 / _FIXED_ONE
    c = ints.to(torch.float64).reshape(k, k) * scale
    total = float(c.sum())
    if not total > 0:
        raise ValueError("multiclass metrics need a positive total weight")
    return MulticlassMetrics(confusion=c, accuracy=float(c.diagonal().sum()) / total,
                             log_loss=float(sums[1] / sums[0]), count=total)


def evaluate(model, shard, comm=None, num_bins: int = 1000, thresholds=None,
             threshold: float = 0.5, *, margins: Optional[torch.Tensor] = None):
    """Evaluate a fitted model on a whole shard of any kind.

    ``LinearModel`` with a logistic or hinge link -> :class:`BinaryMetrics`,
    with the identity link -> :class:`RegressionMetrics`; ``MultinomialModel``
    -> :class:`MulticlassMetrics`. The shard is scored in place
    (``model.score``), its ``sample_weight`` is honoured, and with a
    ``Communicator`` of world size > 1 each rank passes its own row shard and
    every rank returns identical metrics (one int64 and one f64 all-reduce).

    Binary curves are binned: ``num_bins`` (1..4096) bins uniform in sigmoid
    space, edges logit(j / num_bins) — ROC is invariant under monotone maps,
    so the same edges serve hinge models — or explicit strictly increasing
    margin-space ``thresholds``. ``threshold`` is the probability cut of the
    confusion, as in ``LinearModel.predict``. ``margins`` substitutes
    precomputed margins for ``model.score(shard)`` (``[n]``; ``[n, K]`` or
    the class-padded flat buffer for a multinomial model).

    Raises ``ValueError`` on NaN margins, weights that are negative,
    non-finite or sum to 2^31 or more, and a binary shard with one class
    absent globally.
    """
    if hasattr(model, "num_classes"):
        zp = margins if margins is not None else model._score_padded(shard)
        if zp.ndim == 2:  # the logical [n, K] view, as model.score returns it
            from .ops.multiclass import _pad_classes, padded_k

            zp = _pad_classes(zp, padded_k(model.num_classes)).reshape(-1)
        return _evaluate_multiclass(model, shard, zp, comm)
    z = margins if margins is not None else model.score(shard)
    if z.dtype not in (torch.float32, torch.float64):
        z = z.to(torch.float32)
    if model.link == "identity":
        return _evaluate_regression(shard, z, comm)
    if model.link in ("logistic", "hinge"):
        return _evaluate_binary(model, shard, z, comm, num_bins, thresholds,
                                threshold)
    raise ValueError(f"evaluate: unknown link {model.link!r}")
