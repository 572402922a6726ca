"""Shard-native scoring and evaluation on the CPU tier: the metrics oracles,
``model.score`` / ``predict_shard``, ``evaluate`` on every shard kind, sample
weights, input validation and the gloo two-rank reduction."""

import math
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from sparkagd_amd import (
    BinaryMetrics,
    Communicator,
    CSRShard,
    DenseShard,
    HostStreamedDenseShard,
    LinearModel,
    LinearRegressionWithAGD,
    LogisticRegressionWithAGD,
    MixedShard,
    MulticlassMetrics,
    MultinomialModel,
    RegressionMetrics,
    SoftmaxRegressionWithAGD,
    SVMWithAGD,
    evaluate,
    evaluation,
    ops,
)
from sparkagd_amd.data import generate_dense_problem, generate_multiclass_problem
from sparkagd_amd.ops import reference


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def _to_csr(a, y, sample_weight=None):
    sp = a.to_sparse_csr()
    return CSRShard(sp.crow_indices(), sp.col_indices(), sp.values(), y,
                    a.shape[1], sample_weight=sample_weight)


def _grid_problem(n=600, seed=0):
    """A one-feature shard whose margins ARE the feature: values on a 1/8
    grid (plenty of ties), labels correlated with the margin."""
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(n, generator=g) * 1.5 * 8).round() / 8
    y = (z + torch.randn(n, generator=g) > 0).to(torch.float32)
    shard = DenseShard(z.reshape(n, 1).contiguous(), y)
    return shard, LinearModel(torch.ones(1, dtype=torch.float64), [], "logistic")


def _trained(n=1024, d=16, seed=0):
    shard, _ = generate_dense_problem(n=n, d=d, seed=seed, label_noise=1.0)
    return shard, LogisticRegressionWithAGD.train(shard, num_iterations=10)


def _integer_problem(n=300, d=12, seed=7):
    """Small-integer features and 1/8-grid weights: every margin is exact in
    f32 whatever order a kernel or a sparse product sums it in."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-2, 3, (n, d), generator=g).to(torch.float32)
    a[torch.rand(n, d, generator=g) < 0.5] = 0.0
    w = torch.randint(-8, 9, (d,), generator=g).to(torch.float64) / 8
    y = ((a.double() @ w) + torch.randn(n, generator=g).double() > 0).to(torch.float32)
    sw = torch.rand(n, generator=g) * 2
    return a, y, w, sw


# --- 1. binned AUC against the rank statistic ---

def test_auc_with_one_bin_per_distinct_margin_equals_roc_auc():
    shard, model = _grid_problem()
    z = model.score(shard)
    u = torch.unique(z.double())
    assert u.numel() < z.numel() / 4  # ties exist
    m = evaluate(model, shard, thresholds=(u[1:] + u[:-1]) / 2)
    assert isinstance(m, BinaryMetrics)
    assert abs(m.area_under_roc - evaluation.roc_auc(z, shard.labels)) <= 1e-12
    fpr, tpr = m.roc()
    assert (fpr[0], tpr[0], fpr[-1], tpr[-1]) == (0.0, 0.0, 1.0, 1.0)
    assert bool((fpr[1:] >= fpr[:-1]).all()) and bool((tpr[1:] >= tpr[:-1]).all())


@pytest.mark.parametrize("num_bins", [1, 2, 7, 1000, 4096])
def test_binned_auc_equals_roc_auc_of_bin_index(num_bins):
    shard, model = _trained()
    z = model.score(shard)
    m = evaluate(model, shard, num_bins=num_bins)
    assert m.hist_pos.numel() == num_bins and m.edges.numel() == num_bins - 1
    bins = (torch.bucketize(z, m.edges, right=True) if num_bins > 1
            else torch.zeros_like(z, dtype=torch.int64))
    assert abs(m.area_under_roc - evaluation.roc_auc(bins, shard.labels)) <= 1e-12
    assert m.count == shard.n
    assert m.num_positives == float((shard.labels > 0.5).sum())


def test_default_edges_are_uniform_in_sigmoid_space():
    shard, model = _trained()
    m = evaluate(model, shard, num_bins=10)
    torch.testing.assert_close(torch.sigmoid(m.edges.double()),
                               torch.arange(1, 10, dtype=torch.float64) / 10,
                               rtol=0, atol=1e-6)


# --- 2. agreement with the tensor-level metrics ---

@pytest.mark.parametrize("threshold", [0.5, 0.3])
def test_binary_metrics_equal_tensor_functions(threshold):
    shard, model = _trained()
    m = evaluate(model, shard, threshold=threshold)
    pred = model.predict(shard.features, threshold)
    assert torch.equal(pred, model.predict_shard(shard, threshold))
    assert torch.equal(model.score(shard), model.margins(shard.features))
    y = shard.labels > 0.5
    p = pred > 0.5
    want = (float((p & y).sum()), float((p & ~y).sum()),
            float((~p & y).sum()), float((~p & ~y).sum()))
    assert m.confusion == want
    prf = evaluation.precision_recall_f1(pred, shard.labels)
    assert _rel(m.accuracy, evaluation.accuracy(pred, shard.labels)) <= 1e-12
    assert _rel(m.precision, prf["precision"]) <= 1e-12
    assert _rel(m.recall, prf["recall"]) <= 1e-12
    assert _rel(m.f1, prf["f1"]) <= 1e-12
    ll = evaluation.log_loss(model.margins(shard.features), shard.labels)
    assert _rel(m.log_loss, ll) <= 1e-12


def test_hinge_model_has_no_log_loss_and_same_curves():
    shard, _ = generate_dense_problem(n=512, d=8, seed=2, label_noise=1.0)
    model = SVMWithAGD.train(shard, num_iterations=10, reg_param=0.01)
    m = evaluate(model, shard, num_bins=50)
    assert m.log_loss is None
    bins = torch.bucketize(model.score(shard), m.edges, right=True)
    assert abs(m.area_under_roc - evaluation.roc_auc(bins, shard.labels)) <= 1e-12


def test_multiclass_confusion_equals_confusion_matrix():
    k = 5
    shard, _ = generate_multiclass_problem(n=700, d=12, num_classes=k, seed=1)
    model = SoftmaxRegressionWithAGD.train(shard, k, num_iterations=10)
    m = evaluate(model, shard)
    assert isinstance(m, MulticlassMetrics)
    pred = model.predict(shard.features)
    assert torch.equal(pred, model.predict_shard(shard))
    assert torch.equal(model.score(shard), model.margins(shard.features))
    want = evaluation.confusion_matrix(pred, shard.labels, k)
    assert torch.equal(m.confusion, want.to(torch.float64))
    assert _rel(m.accuracy, evaluation.accuracy(pred, shard.labels)) <= 1e-12
    z = model.margins(shard.features).double()
    ll = float((torch.logsumexp(z, 1) - z.gather(
        1, shard.labels.long().unsqueeze(1)).squeeze(1)).mean())
    # f32 margins: the per-row loss is a handful of f32 roundings (6e-8 each)
    assert _rel(m.log_loss, ll) <= 1e-6
    c = want.double()
    for j in range(k):
        assert _rel(m.precision(j), float(c[j, j] / c[:, j].sum())) <= 1e-12
        assert _rel(m.recall(j), float(c[j, j] / c[j].sum())) <= 1e-12
    assert _rel(m.weighted_recall, m.accuracy) <= 1e-12
    assert 0.0 < m.weighted_f1 <= 1.0 and 0.0 < m.weighted_precision <= 1.0


def test_multiclass_csr_shard_scores_like_dense():
    k = 3
    g = torch.Generator().manual_seed(3)
    a = torch.randint(-2, 3, (200, 10), generator=g).to(torch.float32)
    a[torch.rand(200, 10, generator=g) < 0.5] = 0.0
    y = torch.randint(0, k, (200,), generator=g).to(torch.float32)
    w = torch.randint(-8, 9, (10 * k,), generator=g).to(torch.float64) / 8
    model = MultinomialModel(w, [], k)
    md = evaluate(model, DenseShard(a, y))
    ms = evaluate(model, _to_csr(a, y))
    assert torch.equal(md.confusion, ms.confusion)
    assert _rel(md.log_loss, ms.log_loss) <= 1e-9


def test_multiclass_oracle_ties_pick_lowest_index():
    z = torch.tensor([[1.0, 1.0, 0.0, 9.0], [0.0, 2.0, 2.0, 9.0],
                      [3.0, 3.0, 3.0, 9.0]])  # kc = 4, pad column is garbage
    y = torch.tensor([2.0, 2.0, 2.0])
    conf, sums, bad, _ = reference.multiclass_metrics(z.reshape(-1), y, 3, 4)
    assert conf[2].tolist() == [2, 1, 0] and int(bad) == 0
    assert float(sums[0]) == 3.0


# --- 3. integer sample weights == repeated rows ---

def test_integer_weights_equal_repeated_rows():
    # exact margins (see _integer_problem): a row and its copies score the
    # same bits whatever the shape of the product that computes them
    a, y, wm, _ = _integer_problem(n=400)
    shard, model = DenseShard(a, y), LinearModel(wm, [], "logistic")
    g = torch.Generator().manual_seed(5)
    w = torch.randint(0, 4, (shard.n,), generator=g)
    rep = torch.repeat_interleave(torch.arange(shard.n), w)
    weighted = DenseShard(shard.features, shard.labels, w.to(torch.float32))
    repeated = DenseShard(shard.features[rep].contiguous(), shard.labels[rep])
    mw = evaluate(model, weighted, num_bins=64, threshold=0.4)
    mr = evaluate(model, repeated, num_bins=64, threshold=0.4)
    assert torch.equal(mw.hist_pos, mr.hist_pos)
    assert torch.equal(mw.hist_neg, mr.hist_neg)
    assert mw.confusion == mr.confusion and mw.count == mr.count == float(w.sum())
    assert mw.area_under_roc == mr.area_under_roc
    assert mw.area_under_pr == mr.area_under_pr
    assert _rel(mw.log_loss, mr.log_loss) <= 1e-12
    # the raw op: weighted counts are the repeated counts in 2^-32 units
    edges = mw.edges
    ow = ops.binary_metrics(model.score(weighted), weighted.labels, edges, 0.1,
                            weighted.sample_weight)
    orr = ops.binary_metrics(model.score(repeated), repeated.labels, edges, 0.1)
    for a, b in zip(ow[:3], orr[:3]):
        assert a.dtype == torch.int64 and torch.equal(a, b * 2 ** 32)
    torch.testing.assert_close(ow[3], orr[3], rtol=1e-12, atol=0)

    lin = LinearModel(model.weights, [], "identity")
    rw, rr = evaluate(lin, weighted), evaluate(lin, repeated)
    for f in ("mse", "rmse", "mae", "r2", "explained_variance", "count"):
        assert _rel(getattr(rw, f), getattr(rr, f)) <= 1e-12, f


def test_fractional_weights_use_fixed_point_units():
    z = torch.tensor([-1.0, 0.5, 2.0])
    y = torch.tensor([0.0, 1.0, 1.0])
    w = torch.tensor([0.3, 1.7, 0.0])
    hp, hn, conf, sums, nan, wmin = ops.binary_metrics(
        z, y, torch.tensor([0.0]), 0.0, w)
    u = (w.double() * 2 ** 32).round().to(torch.int64)
    assert hp.tolist() == [0, int(u[1] + u[2])] and hn.tolist() == [int(u[0]), 0]
    assert conf.tolist() == [int(u[1] + u[2]), 0, 0, int(u[0])]
    assert int(nan) == 0 and float(wmin) == 0.0
    assert _rel(float(sums[0]), float(w.double().sum())) <= 1e-15


def test_bin_is_the_number_of_edges_at_or_below_the_margin():
    edges = torch.tensor([-1.0, 0.0, 2.0])
    z = torch.tensor([-math.inf, -1.0, -0.0, 0.0, 1.999, 2.0, math.inf])
    y = torch.ones(7)
    hp, hn, conf, sums, nan, _ = ops.binary_metrics(z, y, edges, 0.0)
    assert hp.tolist() == [1, 1, 3, 2] and hn.tolist() == [0, 0, 0, 0]
    assert conf.tolist() == [3, 0, 4, 0]  # z > 0 is strict: ±0.0 are negative
    assert float(sums[1]) == math.inf  # softplus(+inf) for the y=1, z=-inf row


# --- 4. every shard kind ---

@pytest.mark.parametrize("weighted", [False, True])
def test_dense_csr_mixed_streamed_views_agree(weighted):
    a, y, w, sw = _integer_problem()
    sw = sw if weighted else None
    h = 130
    views = {
        "dense": DenseShard(a, y, sw),
        "csr": _to_csr(a, y, sw),
        "mixed": MixedShard([
            DenseShard(a[:h].contiguous(), y[:h], None if sw is None else sw[:h]),
            _to_csr(a[h:].contiguous(), y[h:], None if sw is None else sw[h:])]),
        "streamed": HostStreamedDenseShard(a, y, device="cpu", chunk_rows=64,
                                           sample_weight=sw),
    }
    model = LinearModel(w, [], "logistic")
    ref = evaluate(model, views["dense"], num_bins=32)
    for name, shard in views.items():
        assert torch.equal(model.score(shard).double(), a.double() @ w), name
        m = evaluate(model, shard, num_bins=32)
        assert torch.equal(m.hist_pos, ref.hist_pos), name
        assert torch.equal(m.hist_neg, ref.hist_neg), name
        assert m.confusion == ref.confusion, name
        assert _rel(m.log_loss, ref.log_loss) <= 1e-9, name
        assert _rel(m.count, ref.count) <= 1e-9, name


# --- 5. validation ---

def test_invalid_inputs_raise_value_error():
    shard, model = _trained(n=200)
    with pytest.raises(ValueError, match="num_bins"):
        evaluate(model, shard, num_bins=4097)
    with pytest.raises(ValueError, match="num_bins"):
        evaluate(model, shard, num_bins=0)
    with pytest.raises(ValueError, match="thresholds"):
        evaluate(model, shard, thresholds=torch.arange(4096.0))
    for bad in ([0.0, 0.0], [1.0, 0.5], [0.0, math.nan]):
        with pytest.raises(ValueError, match="strictly increasing"):
            evaluate(model, shard, thresholds=bad)
    f = shard.features.clone()
    f[17, 3] = math.nan
    with pytest.raises(ValueError, match="NaN"):
        evaluate(model, DenseShard(f, shard.labels))
    w = torch.ones(shard.n)
    w[5] = -0.25
    with pytest.raises(ValueError, match="weights"):
        evaluate(model, DenseShard(shard.features, shard.labels, w))
    w[5] = math.inf
    with pytest.raises(ValueError, match="weights"):
        evaluate(model, DenseShard(shard.features, shard.labels, w))
    w[5] = 2.0 ** 31
    with pytest.raises(ValueError, match="weights"):
        evaluate(model, DenseShard(shard.features, shard.labels, w))
    with pytest.raises(ValueError, match="both classes"):
        evaluate(model, DenseShard(shard.features, torch.ones(shard.n)))
    with pytest.raises(ValueError, match="both classes"):
        evaluate(model, DenseShard(shard.features, torch.zeros(shard.n)))


def test_multiclass_label_out_of_range_raises():
    shard, _ = generate_multiclass_problem(n=50, d=4, num_classes=3, seed=0)
    model = MultinomialModel(torch.zeros(12, dtype=torch.float64), [], 3)
    y = shard.labels.clone()
    y[7] = 3.0
    with pytest.raises(ValueError, match="labels outside"):
        evaluate(model, DenseShard(shard.features, y))


# --- 6. gloo world size 2 ---

def _dist_problem():
    shard, _ = generate_dense_problem(n=1024, d=16, seed=11, label_noise=1.0)
    g = torch.Generator().manual_seed(12)
    sw = torch.rand(1024, generator=g) * 3
    w = torch.randn(16, generator=g).double() / 4
    ms, _ = generate_multiclass_problem(n=1024, d=8, num_classes=4, seed=13)
    wm = torch.randn(32, generator=g).double()
    return shard, sw, w, ms, wm


def _metrics_state(m):
    if isinstance(m, BinaryMetrics):
        return {"ints": torch.cat([m.hist_pos, m.hist_neg,
                                   torch.tensor(m.confusion, dtype=torch.float64)]),
                "sums": torch.tensor([m.count, m.log_loss, m.area_under_roc,
                                      m.area_under_pr, m.accuracy, m.f1],
                                     dtype=torch.float64)}
    if isinstance(m, MulticlassMetrics):
        return {"ints": m.confusion.reshape(-1),
                "sums": torch.tensor([m.count, m.log_loss, m.accuracy,
                                      m.weighted_f1], dtype=torch.float64)}
    return {"ints": torch.zeros(0, dtype=torch.float64),
            "sums": torch.tensor([m.mse, m.mae, m.r2, m.explained_variance,
                                  m.count], dtype=torch.float64)}


def _all_metrics(lo, hi, comm):
    shard, sw, w, ms, wm = _dist_problem()
    f, y = shard.features[lo:hi].contiguous(), shard.labels[lo:hi]
    out = {
        "plain": evaluate(LinearModel(w, [], "logistic"), DenseShard(f, y), comm,
                          num_bins=100),
        "weighted": evaluate(LinearModel(w, [], "logistic"),
                             _to_csr(f, y, sw[lo:hi]), comm, num_bins=100),
        "regression": evaluate(LinearModel(w, [], "identity"),
                               DenseShard(f, y, sw[lo:hi]), comm),
        "multi": evaluate(MultinomialModel(wm, [], 4),
                          DenseShard(ms.features[lo:hi].contiguous(),
                                     ms.labels[lo:hi], sw[lo:hi]), comm),
    }
    return {k: _metrics_state(v) for k, v in out.items()}


def _dist_worker(rank, world, init_file, out_dir):
    torch.distributed.init_process_group(
        "gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    try:
        lo, hi = (0, 700) if rank == 0 else (700, 1024)  # uneven split
        torch.save(_all_metrics(lo, hi, Communicator()),
                   os.path.join(out_dir, f"r{rank}.pt"))
    finally:
        torch.distributed.destroy_process_group()


def test_two_rank_metrics_identical_and_match_single_process():
    fd, init_file = tempfile.mkstemp(prefix="sparkagd_eval_", suffix=".init")
    os.close(fd)
    os.unlink(init_file)
    with tempfile.TemporaryDirectory() as out_dir:
        mp.spawn(_dist_worker, args=(2, init_file, out_dir), nprocs=2, join=True)
        r0 = torch.load(os.path.join(out_dir, "r0.pt"))
        r1 = torch.load(os.path.join(out_dir, "r1.pt"))
    if os.path.exists(init_file):
        os.unlink(init_file)
    single = _all_metrics(0, 1024, None)
    for kind in single:
        for part in ("ints", "sums"):
            a, b = r0[kind][part], r1[kind][part]
            assert torch.equal(a.view(torch.int64), b.view(torch.int64)), (kind, part)
        assert torch.equal(r0[kind]["ints"], single[kind]["ints"]), kind
        torch.testing.assert_close(r0[kind]["sums"], single[kind]["sums"],
                                   rtol=1e-12, atol=0, msg=kind)


# --- 7. regression ---

def test_regression_metrics_closed_form():
    shard, _ = generate_dense_problem(n=333, d=9, seed=4,
                                      loss_type=ops.LOSS_LEAST_SQUARES)
    g = torch.Generator().manual_seed(9)
    sw = torch.rand(333, generator=g) + 0.5
    model = LinearRegressionWithAGD.train(shard, num_iterations=5)
    for weights in (None, sw):
        m = evaluate(model, DenseShard(shard.features, shard.labels, weights))
        assert isinstance(m, RegressionMetrics)
        z = model.margins(shard.features).double().numpy()
        y = shard.labels.double().numpy()
        w = np.ones_like(y) if weights is None else weights.double().numpy()
        res = y - z
        mse = np.average(res ** 2, weights=w)
        ybar = np.average(y, weights=w)
        var_y = np.average((y - ybar) ** 2, weights=w)
        var_res = np.average((res - np.average(res, weights=w)) ** 2, weights=w)
        assert _rel(m.mse, mse) <= 1e-10
        assert _rel(m.rmse, math.sqrt(mse)) <= 1e-10
        assert _rel(m.mae, np.average(np.abs(res), weights=w)) <= 1e-10
        assert _rel(m.r2, 1.0 - mse / var_y) <= 1e-9
        assert _rel(m.explained_variance, 1.0 - var_res / var_y) <= 1e-9
        assert _rel(m.count, w.sum()) <= 1e-12


# --- curves ---

def test_pr_curve_and_f_measure_by_threshold():
    shard, model = _grid_problem(n=400, seed=3)
    z = model.score(shard).double()
    u = torch.unique(z)
    m = evaluate(model, shard, thresholds=(u[1:] + u[:-1]) / 2)
    rec, prec = m.pr()
    y = shard.labels > 0.5
    # brute force over the distinct scores, top down
    want_r, want_p = [], []
    for t in u.flip(0):
        p = z >= t
        want_r.append(float((p & y).sum()) / float(y.sum()))
        want_p.append(float((p & y).sum()) / float(p.sum()))
    torch.testing.assert_close(rec[1:], torch.tensor(want_r, dtype=torch.float64),
                               rtol=1e-12, atol=0)
    torch.testing.assert_close(prec[1:], torch.tensor(want_p, dtype=torch.float64),
                               rtol=1e-12, atol=0)
    assert float(rec[0]) == 0.0 and float(prec[0]) == want_p[0]
    assert 0.5 < m.area_under_pr <= 1.0
    thr, f1 = m.f_measure_by_threshold()
    assert thr.numel() == f1.numel() == u.numel() and float(thr[-1]) == -math.inf
    want_f = [2 * p * r / (p + r) if p + r > 0 else 0.0
              for p, r in zip(want_p, want_r)]
    torch.testing.assert_close(f1, torch.tensor(want_f, dtype=torch.float64),
                               rtol=1e-12, atol=0)
    _, f2 = m.f_measure_by_threshold(beta=2.0)
    assert float(f2[-1]) > float(f1[-1])  # recall 1 at the bottom favours beta=2


# --- the example ---

def test_evaluate_sharded_example_runs():
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(
        [sys.executable, os.path.join(repo, "examples", "evaluate_sharded.py"),
         "--n", "1000", "--d", "32", "--iters", "10"],
        capture_output=True, text=True, timeout=300, cwd=repo)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "evaluation OK" in out.stdout
    for tag in ("CSR logistic", "dense lsq", "dense softmax"):
        assert tag in out.stdout
