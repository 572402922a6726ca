"""One-vs-rest multiclass training — CPU tier, f64: the stacked evaluation
against K relabelled binary evaluations, and the trainer end to end."""

import pytest
import torch

from sparkagd_amd import (
    DenseShard, LeastSquaresGradient, LogisticGradient, MultiTaskGradient,
    OneVsRestModel, OneVsRestWithAGD, SmoothedHingeGradient,
)

K = 3


def _blobs(n=300, d=8, seed=0):
    """Three Gaussian blobs, centres 6 apart on the first three axes."""
    g = torch.Generator().manual_seed(seed)
    labels = torch.arange(n) % K
    x = 0.5 * torch.randn(n, d, generator=g, dtype=torch.float64)
    x[torch.arange(n), labels] += 6.0
    return DenseShard(x, labels.to(torch.float32))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("grad_cls", [LogisticGradient, SmoothedHingeGradient,
                                      LeastSquaresGradient])
def test_eval_is_k_relabelled_binary_evals(grad_cls, weighted):
    shard = _blobs(n=91, d=7, seed=1)
    g = torch.Generator().manual_seed(2)
    sw = 0.5 + torch.rand(shard.n, generator=g) if weighted else None
    shard = DenseShard(shard.features, shard.labels, sw)
    w = 0.3 * torch.randn(shard.d * K, generator=g, dtype=torch.float64)
    ovr = MultiTaskGradient(grad_cls(), K, sample_weight=sw,
                            target_class=range(K))
    grad, lc = ovr.eval(shard, w)
    loss = 0.0
    for c in range(K):
        sub = DenseShard(shard.features, (shard.labels == c).to(torch.float32), sw)
        g_c, lc_c = grad_cls().eval(sub, w.reshape(-1, K)[:, c].contiguous())
        torch.testing.assert_close(grad.reshape(-1, K)[:, c], g_c,
                                   rtol=1e-12, atol=0.0)
        torch.testing.assert_close(ovr.last_task_loss[c], lc_c[0],
                                   rtol=1e-12, atol=0.0)
        assert float(lc[1]) == float(lc_c[1])
        loss += float(lc_c[0])
    assert abs(float(lc[0]) - loss) <= 1e-12 * abs(loss)


@pytest.mark.parametrize("loss", ["logistic", "hinge"])
def test_train_separates_blobs_and_round_trips(loss, tmp_path):
    shard = _blobs()
    model = OneVsRestWithAGD.train(shard, K, loss=loss, num_iterations=60,
                                   reg_param=[1e-3, 2e-3, 5e-3])
    assert model.weights.shape == (shard.d, K)
    assert torch.equal(model.predict(shard), shard.labels)
    assert model.score(shard).shape == (shard.n, K)
    path = str(tmp_path / "ovr.safetensors")
    model.save(path)
    back = OneVsRestModel.load(path)
    assert torch.equal(back.weights, model.weights)
    assert (back.num_classes, back.link) == (K, model.link)
    assert back.loss_history == model.loss_history


def test_predict_gives_ties_to_the_lowest_class():
    shard = _blobs(n=6)
    model = OneVsRestModel(torch.zeros(shard.d, K, dtype=torch.float64), [], K,
                           "logistic")
    assert torch.equal(model.predict(shard), torch.zeros(shard.n))


def test_train_rejects_bad_labels_and_reg_param():
    shard = _blobs(n=30)
    for bad in (3.0, -1.0, 0.5):
        labels = shard.labels.clone()
        labels[4] = bad
        with pytest.raises(ValueError, match="class indices"):
            OneVsRestWithAGD.train(DenseShard(shard.features, labels), K,
                                   num_iterations=1)
    with pytest.raises(ValueError, match="one value per class"):
        OneVsRestWithAGD.train(shard, K, reg_param=[0.1, 0.2], num_iterations=1)
    with pytest.raises(ValueError, match="one entry per task"):
        MultiTaskGradient(LogisticGradient(), K, target_class=[0, 1])
    with pytest.raises(ValueError, match="class ids"):
        MultiTaskGradient(LogisticGradient(), K, target_class=[0, -1, 2])
