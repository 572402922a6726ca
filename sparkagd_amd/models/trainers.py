"""User-layer model trainers (the reference's L6).

In the reference this layer is MLlib's trainer classes (e.g.
``LogisticRegressionWithSGD``-style wrappers) that construct an optimizer and
call ``optimize()`` (in-repo example
``AcceleratedGradientDescentSuite.scala:217-222``). These are the equivalent
conveniences: a GLM trainer per loss family, returning a fitted linear model
with ``predict``.
"""

from __future__ import annotations

from typing import Optional, Union

import torch

from ..config import AGDConfig
from ..optimizer import AcceleratedGradientDescent
from ..parallel.comm import Communicator
from .gradient import HingeGradient, LeastSquaresGradient, LogisticGradient
from .updater import SimpleUpdater, SquaredL2Updater, Updater


def _save_model(path: str, weights: torch.Tensor, meta: dict) -> None:
    import json
    import os as _os
    import tempfile

    from safetensors.torch import save_file

    d = _os.path.dirname(_os.path.abspath(path)) or "."
    _os.makedirs(d, exist_ok=True)
    fd, tmp = tempfile.mkstemp(dir=d, suffix=".tmp")
    _os.close(fd)
    try:
        save_file({"weights": weights.detach().cpu().contiguous().clone()},
                  tmp, metadata={k: json.dumps(v) for k, v in meta.items()})
        _os.replace(tmp, path)
    finally:
        if _os.path.exists(tmp):
            _os.unlink(tmp)


def _load_model(path: str, device=None):
    import json

    from safetensors import safe_open
    from safetensors.torch import load_file

    with safe_open(path, framework="pt", device="cpu") as f:
        meta = {k: json.loads(v) for k, v in (f.metadata() or {}).items()}
    w = load_file(path)["weights"]
    if device is not None:
        w = w.to(device)
    return w, meta


def _shard_feature_dtype(shard) -> torch.dtype:
    if getattr(shard, "kind", None) == "mixed":
        dts = [_shard_feature_dtype(p) for p in shard.parts]
        return torch.float64 if torch.float64 in dts else dts[0]
    if getattr(shard, "kind", None) == "dense_streamed":
        return shard.feature_dtype  # features_host may be released
    for attr in ("features", "val"):
        t = getattr(shard, attr, None)
        if t is not None:
            return t.dtype
    raise TypeError(f"unsupported shard type {type(shard).__name__}")


def _weights_for(shard, weights: torch.Tensor) -> torch.Tensor:
    """The model weights placed and typed as ``shard.margins`` wants them:
    on the shard's device, and on GPU in the kernels' accumulator dtype (f64
    for f64 features, f32 for everything narrower)."""
    dev = torch.device(shard.device)
    w = weights.to(dev)
    if dev.type == "cuda":
        f64 = _shard_feature_dtype(shard) == torch.float64
        w = w.to(torch.float64 if f64 else torch.float32)
    return w.contiguous()


def _with_intercept(data, updater: Updater, initial_weights, initial_intercept: float):
    """``intercept=True`` plumbing shared by the trainers: the shard wrapped
    in an ``InterceptShard``, the updater in a ``FreeTailUpdater`` and the
    start vector extended to ``[w; b]``."""
    from ..data import InterceptShard
    from .updater import FreeTailUpdater

    data = InterceptShard(data)
    if not isinstance(updater, FreeTailUpdater):
        updater = FreeTailUpdater(updater, 1)
    elif updater.n_free != 1:
        raise ValueError("intercept=True needs a FreeTailUpdater with n_free=1")
    if initial_weights is not None:
        if initial_weights.numel() != data.d - 1:
            raise ValueError(
                f"initial_weights must be [{data.d - 1}] (the intercept is "
                "given by initial_intercept)")
        bias = torch.full((1,), float(initial_intercept),
                          dtype=initial_weights.dtype,
                          device=initial_weights.device)
        initial_weights = torch.cat([initial_weights.reshape(-1), bias])
    elif initial_intercept != 0.0:
        wdtype = torch.float64 if data.device.type == "cpu" else torch.float32
        initial_weights = torch.zeros(data.d, device=data.device, dtype=wdtype)
        initial_weights[-1] = float(initial_intercept)
    return data, updater, initial_weights


def _split_intercept(w: torch.Tensor):
    """``[w; b]`` -> (w [d] as its own tensor, b as a float)."""
    return w[:-1].clone(), float(w[-1])


class LinearModel:
    """A fitted generalized linear model: weights [d], an ``intercept``
    (0.0 for a model trained without one) and the loss history.
    MLlib-style model persistence via ``save``/``load`` (safetensors)."""

    def __init__(self, weights: torch.Tensor, loss_history, link: str,
                 intercept: float = 0.0):
        self.weights = weights
        self.loss_history = list(loss_history)
        self.link = link
        self.intercept = float(intercept)

    def save(self, path: str) -> None:
        _save_model(path, self.weights, {"kind": "linear", "link": self.link,
                                         "loss_history": self.loss_history,
                                         "intercept": self.intercept})

    @classmethod
    def load(cls, path: str, device=None) -> "LinearModel":
        w, meta = _load_model(path, device)
        if meta.get("kind") != "linear":
            raise ValueError(f"not a LinearModel checkpoint: {meta.get('kind')}")
        return cls(w, meta.get("loss_history", []), meta["link"],
                   meta.get("intercept", 0.0))

    def margins(self, features: torch.Tensor) -> torch.Tensor:
        acc = torch.float32 if features.dtype in (torch.bfloat16, torch.float16) else features.dtype
        z = features.to(acc) @ self.weights.to(acc)
        if self.intercept != 0.0:
            z = z + self.intercept
        return z

    def predict(self, features: torch.Tensor,
                threshold: Optional[float] = 0.5) -> torch.Tensor:
        """Class predictions. ``threshold`` is the probability cut for
        logistic models (MLlib's ``setThreshold`` analog; margin cut
        logit(t)); ``None`` returns the raw margin (``clearThreshold``
        semantics). Identity-link models always return the raw prediction."""
        import math as _math

        z = self.margins(features)
        if self.link == "identity":
            return z
        if threshold is None:
            return z
        cut = 0.0
        if self.link == "logistic" and threshold != 0.5:
            cut = _math.log(threshold / (1.0 - threshold))
        return (z > cut).to(torch.float32)

    def predict_proba(self, features: torch.Tensor) -> torch.Tensor:
        if self.link != "logistic":
            raise ValueError("predict_proba only for logistic models")
        return torch.sigmoid(self.margins(features))

    def _cut(self, threshold: float) -> float:
        """Margin-space cut of a probability threshold (see ``predict``)."""
        import math as _math

        if self.link == "logistic" and threshold != 0.5:
            return _math.log(threshold / (1.0 - threshold))
        return 0.0

    def score(self, shard) -> torch.Tensor:
        """Margins [n] of a whole shard of any kind (dense bf16 / f32 / f64 /
        fp8, CSR, mixed, host-streamed) through the shard's own
        ``margins`` kernels — the features are read in place, never copied
        or widened. The model's ``intercept`` is added when it is not 0."""
        z = shard.margins(_weights_for(shard, self.weights))
        if self.intercept != 0.0:
            z = z + self.intercept
        return z

    def predict_shard(self, shard,
                      threshold: Optional[float] = 0.5) -> torch.Tensor:
        """``predict`` over a shard: same thresholds, same strict ``z > cut``
        comparison, margins from ``score``."""
        z = self.score(shard)
        if self.link == "identity" or threshold is None:
            return z
        return (z > self._cut(threshold)).to(torch.float32)


class _GLMTrainer:
    GRADIENT_CLS = LogisticGradient
    LINK = "logistic"

    @classmethod
    def train(
        cls,
        data,
        num_iterations: int = 100,
        reg_param: float = 0.0,
        convergence_tol: float = 1e-4,
        updater: Optional[Updater] = None,
        initial_weights: Optional[torch.Tensor] = None,
        comm: Optional[Communicator] = None,
        config: Optional[AGDConfig] = None,
        checkpoint_path: Optional[str] = None,
        checkpoint_every: int = 0,
        resume_from: Optional[str] = None,
        feature_scaling: Union[bool, str] = False,
        intercept: bool = False,
        initial_intercept: float = 0.0,
    ) -> LinearModel:
        """Fit the model. ``intercept=True`` (MLlib's ``setIntercept``) also
        fits a bias, returned as ``model.intercept``: it is carried natively
        (:class:`~sparkagd_amd.data.InterceptShard`, no ones column, any
        shard kind but host-streamed) and never regularised — ``updater``,
        default or given, is wrapped in a
        :class:`~sparkagd_amd.models.updater.FreeTailUpdater`.
        ``initial_intercept`` is its starting value; ``initial_weights`` stay
        ``[d]``.

        ``feature_scaling`` (default ``False``: the data is
        used as is) standardises the columns first, as MLlib's GLM trainers
        do (``useFeatureScaling``): ``True`` fits a
        :class:`~sparkagd_amd.stats.StandardScaler`, trains on an
        out-of-place scaled copy of the shard (a second copy of a dense
        shard's features, or of a CSR shard's two value arrays, lives for the
        duration of training) and returns a model whose ``weights`` are
        already mapped back to the original feature space, so ``predict`` on
        raw features needs no scaler. ``"inplace"`` does the same but
        overwrites the caller's shard — for shards near memory capacity. As in
        MLlib the regulariser acts on the scaled-space weights, and the loss
        history is the scaled-space objective. ``initial_weights`` are always
        given in the original space."""
        from ..stats import scaled_training_data

        data, scaler, initial_weights = scaled_training_data(
            data, feature_scaling, comm, initial_weights)
        cfg = config or AGDConfig()
        cfg.num_iterations = num_iterations
        cfg.reg_param = reg_param
        cfg.convergence_tol = convergence_tol
        if updater is None:
            updater = SquaredL2Updater() if reg_param > 0 else SimpleUpdater()
        if intercept:
            data, updater, initial_weights = _with_intercept(
                data, updater, initial_weights, initial_intercept)
        opt = AcceleratedGradientDescent(cls.GRADIENT_CLS(), updater, cfg, comm)
        opt.checkpoint_path = checkpoint_path
        opt.checkpoint_every = checkpoint_every
        opt.resume_from = resume_from
        if initial_weights is None:
            wdtype = torch.float64 if data.device.type == "cpu" else torch.float32
            initial_weights = torch.zeros(data.d, device=data.device, dtype=wdtype)
        w = opt.optimize(data, initial_weights)
        bias = 0.0
        if intercept:
            # no centring in the scaler, so the bias needs no mapping
            w, bias = _split_intercept(w)
        if scaler is not None:
            w = scaler.unscale_weights(w)
        return LinearModel(w, opt.loss_history, cls.LINK, bias)


def regularization_path(
    data,
    lambdas,
    gradient=None,
    num_iterations: int = 100,
    convergence_tol: float = 1e-6,
    solver: str = "auto",
    comm: Optional[Communicator] = None,
    warm_start: bool = True,
    intercept: bool = False,
):
    """Solve an L2 regularization path (one model per lambda), reusing the
    Gram operator across solves when eligible — hyperparameter sweeps then
    cost O(n_local·n_global) per solve instead of full shard passes
    (sparkagd_amd/gram.py). Returns a list of LinearModel, one per lambda.

    solver: 'auto' uses the Gram solver for dense shards (falling back to
    direct if K exceeds the memory budget), 'direct'/'gram' force a path.

    intercept: also fit an unregularised bias (``model.intercept``) at every
    lambda, warm-started along the path like the weights. Binary losses and
    the direct solver only ('auto' selects it; 'gram' raises).
    """
    from ..gram import GramOperator
    from ..optimizer import run

    gradient = gradient or LogisticGradient()
    updater = SquaredL2Updater()
    is_multi = getattr(gradient, "IS_MULTICLASS", False)
    if intercept:
        if is_multi:
            raise ValueError("intercept=True supports the binary losses only")
        if solver == "gram":
            raise ValueError(
                "intercept=True needs the direct solver (solver='auto' or "
                "'direct')")
        solver = "direct"
        data, updater, _ = _with_intercept(data, updater, None, 0.0)
    link = {0: "logistic", 1: "identity", 2: "hinge", 3: "hinge"}.get(
        gradient.LOSS_TYPE, "logistic")
    comm = comm or Communicator()
    op = None
    if solver in ("auto", "gram") and getattr(data, "kind", None) == "dense":
        try:
            op = GramOperator(data, comm)
        except MemoryError:
            if solver == "gram":
                raise
            op = None
    wdtype = torch.float64 if data.device.type == "cpu" else torch.float32
    dim = data.d * gradient.num_classes if is_multi else data.d
    w = torch.zeros(dim, device=data.device, dtype=wdtype)
    models = []
    for lam in lambdas:
        w0 = w if warm_start else torch.zeros_like(w)
        import math as _math

        w, hist = run(
            data, gradient, updater, convergence_tol, num_iterations,
            float(lam), w0, 1.0, _math.inf, 0.5, 0.9, True,
            loss_history_mode="backtrack", comm=comm,
            solver="gram" if op is not None else "direct", gram_op=op,
        )
        if is_multi:
            models.append(MultinomialModel(w.clone(), hist,
                                           gradient.num_classes))
        elif intercept:
            wd, bias = _split_intercept(w)
            models.append(LinearModel(wd, hist, link, bias))
        else:
            models.append(LinearModel(w.clone(), hist, link))
    return models


class MultinomialModel:
    """A fitted softmax (multinomial logistic) model: weights [d*K]
    feature-major. predict returns class indices; predict_proba softmax
    probabilities [n, K]."""

    def __init__(self, weights: torch.Tensor, loss_history, num_classes: int):
        self.weights = weights
        self.loss_history = list(loss_history)
        self.num_classes = int(num_classes)

    def margins(self, features: torch.Tensor) -> torch.Tensor:
        acc = torch.float32 if features.dtype in (torch.bfloat16, torch.float16) else features.dtype
        w = self.weights.reshape(features.shape[1], self.num_classes).to(acc)
        return features.to(acc) @ w  # [n, K]

    def predict(self, features: torch.Tensor) -> torch.Tensor:
        return self.margins(features).argmax(dim=1).to(torch.float32)

    def predict_proba(self, features: torch.Tensor) -> torch.Tensor:
        return torch.softmax(self.margins(features), dim=1)

    def _score_padded(self, shard) -> torch.Tensor:
        from .gradient import MultinomialLogisticGradient

        return MultinomialLogisticGradient(self.num_classes).margins(
            shard, _weights_for(shard, self.weights))

    def score(self, shard) -> torch.Tensor:
        """Margins of a whole dense or CSR shard as the logical [n, K] view
        of the kernels' class-padded buffer; the features are read in place."""
        from ..ops.multiclass import padded_k

        zp = self._score_padded(shard)
        return zp.reshape(shard.n, padded_k(self.num_classes))[:, :self.num_classes]

    def predict_shard(self, shard, threshold: Optional[float] = 0.5) -> torch.Tensor:
        """``predict`` over a shard (class indices as f32). ``threshold`` is
        accepted for signature parity with ``LinearModel`` and has no effect
        on an argmax."""
        return self.score(shard).argmax(dim=1).to(torch.float32)

    def save(self, path: str) -> None:
        _save_model(path, self.weights,
                    {"kind": "multinomial", "num_classes": self.num_classes,
                     "loss_history": self.loss_history})

    @classmethod
    def load(cls, path: str, device=None) -> "MultinomialModel":
        w, meta = _load_model(path, device)
        if meta.get("kind") != "multinomial":
            raise ValueError(f"not a MultinomialModel checkpoint: {meta.get('kind')}")
        return cls(w, meta.get("loss_history", []), meta["num_classes"])


class SoftmaxRegressionWithAGD:
    """Multinomial (softmax) logistic regression trainer — a model family
    beyond the reference (MLlib 1.3's LogisticGradient is binary-only)."""

    @classmethod
    def train(
        cls,
        data,
        num_classes: int,
        num_iterations: int = 100,
        reg_param: float = 0.0,
        convergence_tol: float = 1e-4,
        updater: Optional[Updater] = None,
        initial_weights: Optional[torch.Tensor] = None,
        comm: Optional[Communicator] = None,
        config: Optional[AGDConfig] = None,
        feature_scaling: Union[bool, str] = False,
    ) -> MultinomialModel:
        """``feature_scaling``: ``False`` | ``True`` | ``"inplace"``, as in
        the binary GLM trainers (column standardisation before optimising;
        ``True`` holds a scaled copy of the features during training; the
        regulariser acts on the scaled-space weights; returned weights and
        ``initial_weights`` are in the original feature space)."""
        from ..stats import scaled_training_data
        from .gradient import MultinomialLogisticGradient

        data, scaler, initial_weights = scaled_training_data(
            data, feature_scaling, comm, initial_weights, num_classes)

        cfg = config or AGDConfig()
        cfg.num_iterations = num_iterations
        cfg.reg_param = reg_param
        cfg.convergence_tol = convergence_tol
        if updater is None:
            updater = SquaredL2Updater() if reg_param > 0 else SimpleUpdater()
        opt = AcceleratedGradientDescent(
            MultinomialLogisticGradient(num_classes), updater, cfg, comm)
        if initial_weights is None:
            wdtype = torch.float64 if data.device.type == "cpu" else torch.float32
            initial_weights = torch.zeros(data.d * num_classes,
                                          device=data.device, dtype=wdtype)
        w = opt.optimize(data, initial_weights)
        if scaler is not None:
            w = scaler.unscale_weights(w, num_classes)
        return MultinomialModel(w, opt.loss_history, num_classes)


class _SGDTrainer:
    """MLlib 1.3's primary entry points were ``LogisticRegressionWithSGD``
    etc. (``GradientDescent``-backed); these are the equivalents, returning
    the same fitted ``LinearModel`` as the AGD trainers."""

    GRADIENT_CLS = LogisticGradient
    LINK = "logistic"

    @classmethod
    def train(
        cls,
        data,
        num_iterations: int = 100,
        step_size: float = 1.0,
        mini_batch_fraction: float = 1.0,
        reg_param: float = 0.0,
        updater: Optional[Updater] = None,
        initial_weights: Optional[torch.Tensor] = None,
        comm: Optional[Communicator] = None,
        step_schedule: str = "sqrt",
        feature_scaling: Union[bool, str] = False,
        intercept: bool = False,
        initial_intercept: float = 0.0,
    ) -> LinearModel:
        """``feature_scaling``: ``False`` | ``True`` | ``"inplace"``, as in
        the AGD trainers (column standardisation before optimising; ``True``
        holds a scaled copy of the features during training; the regulariser
        acts on the scaled-space weights; returned weights and
        ``initial_weights`` are in the original feature space).
        ``intercept`` / ``initial_intercept``: a native, unregularised bias,
        as in the AGD trainers."""
        from ..optimizer import GradientDescent
        from ..stats import scaled_training_data

        data, scaler, initial_weights = scaled_training_data(
            data, feature_scaling, comm, initial_weights)

        if updater is None:
            updater = SquaredL2Updater() if reg_param > 0 else SimpleUpdater()
        if intercept:
            data, updater, initial_weights = _with_intercept(
                data, updater, initial_weights, initial_intercept)
        opt = (GradientDescent(cls.GRADIENT_CLS(), updater, comm)
               .setStepSize(step_size).setNumIterations(num_iterations)
               .setRegParam(reg_param).setMiniBatchFraction(mini_batch_fraction)
               .setStepSchedule(step_schedule))
        if initial_weights is None:
            wdtype = torch.float64 if data.device.type == "cpu" else torch.float32
            initial_weights = torch.zeros(data.d, device=data.device, dtype=wdtype)
        w = opt.optimize(data, initial_weights)
        bias = 0.0
        if intercept:
            w, bias = _split_intercept(w)
        if scaler is not None:
            w = scaler.unscale_weights(w)
        return LinearModel(w, opt.loss_history, cls.LINK, bias)


class LogisticRegressionWithSGD(_SGDTrainer):
    GRADIENT_CLS = LogisticGradient
    LINK = "logistic"


class LinearRegressionWithSGD(_SGDTrainer):
    GRADIENT_CLS = LeastSquaresGradient
    LINK = "identity"


class SVMWithSGD(_SGDTrainer):
    GRADIENT_CLS = HingeGradient
    LINK = "hinge"


class LogisticRegressionWithAGD(_GLMTrainer):
    GRADIENT_CLS = LogisticGradient
    LINK = "logistic"


class LinearRegressionWithAGD(_GLMTrainer):
    GRADIENT_CLS = LeastSquaresGradient
    LINK = "identity"


class SVMWithAGD(_GLMTrainer):
    GRADIENT_CLS = HingeGradient
    LINK = "hinge"
