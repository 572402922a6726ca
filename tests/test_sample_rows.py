"""The ``sample_rows`` knob of the mini-batch optimizer on the CPU, where both
ways are plain f64 torch over the same rows."""

import pytest
import torch

from sparkagd_amd import (CSRShard, DenseShard, GradientDescent,
                          HostStreamedDenseShard, InterceptShard,
                          LogisticGradient, LogisticRegressionWithSGD,
                          MixedShard, MultinomialLogisticGradient,
                          SimpleUpdater, run_mini_batch)
from sparkagd_amd.data import generate_csr_problem, generate_dense_problem
from sparkagd_amd.models.updater import FreeTailUpdater


class _BatchSizes:
    def __init__(self):
        self.sizes = []

    def log(self, **kw):
        self.sizes.append(kw["batch_size"])


def _dense64(n=200, d=24):
    shard, _ = generate_dense_problem(n, d, seed=5, dtype=torch.float64)
    return shard


def _run(data, updater, fraction, **kw):
    rec = _BatchSizes()
    w0 = torch.zeros(data.d, dtype=torch.float64)
    w, hist = run_mini_batch(data, LogisticGradient(), updater, 1.0, 15, 0.0,
                             fraction, w0, metrics=rec, **kw)
    return w, hist, rec.sizes


@pytest.mark.parametrize("intercept", [False, True], ids=["dense", "intercept"])
def test_sample_rows_reproduces_masked_run(intercept):
    data, upd = _dense64(), SimpleUpdater()
    if intercept:
        data, upd = InterceptShard(data), FreeTailUpdater(upd)
    w_off, h_off, b_off = _run(data, upd, 0.3)
    w_on, h_on, b_on = _run(data, upd, 0.3, sample_rows=True)
    assert b_on == b_off and len(h_on) == len(h_off) == 15
    assert h_on == pytest.approx(h_off, rel=1e-12)
    assert torch.allclose(w_on, w_off, rtol=1e-10, atol=1e-12)


def test_fraction_one_ignores_the_knob():
    csr, _ = generate_csr_problem(50, 16, 4, seed=1)
    for data in (_dense64(), csr):  # also on a kind the knob does not serve
        w_off, h_off, _ = _run(data, SimpleUpdater(), 1.0)
        w_on, h_on, _ = _run(data, SimpleUpdater(), 1.0, sample_rows=True)
        assert torch.equal(w_on, w_off) and h_on == h_off


def test_setters_and_trainers_pass_the_knob():
    data = _dense64()
    w0 = torch.zeros(data.d, dtype=torch.float64)
    opt = (GradientDescent(LogisticGradient(), SimpleUpdater())
           .setNumIterations(5).setMiniBatchFraction(0.5).setSampleRows(True))
    assert opt.sample_rows is True
    opt.optimize(data, w0)
    ref = (GradientDescent(LogisticGradient(), SimpleUpdater())
           .setNumIterations(5).setMiniBatchFraction(0.5))
    ref.optimize(data, w0)
    assert opt.loss_history == pytest.approx(ref.loss_history, rel=1e-12)
    m = LogisticRegressionWithSGD.train(data, 5, mini_batch_fraction=0.5,
                                        sample_rows=True)
    assert list(m.loss_history) == pytest.approx(ref.loss_history, rel=1e-12)


def test_unsupported_kinds_raise():
    dense = _dense64(40, 8)
    csr, _ = generate_csr_problem(40, 8, 3, seed=2)
    kinds = [csr, InterceptShard(csr), MixedShard([dense, csr]),
             HostStreamedDenseShard(dense.features, dense.labels, device="cpu")]
    for data in kinds:
        with pytest.raises(ValueError, match="resident DenseShard"):
            _run(data, SimpleUpdater(), 0.5, sample_rows=True)
    with pytest.raises(ValueError, match="binary loss"):
        run_mini_batch(dense, MultinomialLogisticGradient(3), SimpleUpdater(),
                       1.0, 2, 0.0, 0.5,
                       torch.zeros(dense.d * 3, dtype=torch.float64),
                       sample_rows=True)
