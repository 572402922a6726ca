"""Column statistics and feature standardisation: oracle and API semantics
on CPU (the f64 oracle path); the HIP kernels are covered by
``test_gpu_stats.py``."""

import math
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from sparkagd_amd import (
    ColumnSummary,
    Communicator,
    CSRShard,
    DenseShard,
    HostStreamedDenseShard,
    LogisticRegressionWithAGD,
    MixedShard,
    SoftmaxRegressionWithAGD,
    StandardScaler,
    column_stats,
    generate_dense_problem,
    ops,
)
from sparkagd_amd.ops import reference


def _pin_matrix() -> np.ndarray:
    """7x5, every entry exactly representable in bf16: col 0 generic, col 1
    all zero, col 2 constant, col 3 with some zeros, col 4 negative values."""
    return np.array([
        [1.5, 0.0, 3.0, 0.0, -2.0],
        [-0.25, 0.0, 3.0, 4.0, -1.0],
        [2.0, 0.0, 3.0, 0.0, -8.0],
        [0.5, 0.0, 3.0, -1.5, -0.5],
        [8.0, 0.0, 3.0, 0.0, -4.0],
        [-3.0, 0.0, 3.0, 2.0, -0.125],
        [0.75, 0.0, 3.0, 0.0, -16.0],
    ], dtype=np.float64)


def _to_csr(a: torch.Tensor, labels: torch.Tensor, dense_cols=(),
            deterministic=True) -> CSRShard:
    """CSR shard storing the non-zeros of ``a`` (and every entry of
    ``dense_cols``, zeros included)."""
    n, d = a.shape
    keep = a != 0
    for c in dense_cols:
        keep[:, c] = True
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = keep.sum(dim=1).cumsum(0)
    r, c = torch.nonzero(keep, as_tuple=True)
    return CSRShard(rowptr, c.to(torch.int32), a[r, c].contiguous(), labels, d,
                    deterministic=deterministic)


def _labels(n: int) -> torch.Tensor:
    return (torch.arange(n) % 2).to(torch.float32)


def _assert_summary_close(a: ColumnSummary, b: ColumnSummary, tol=1e-12):
    assert a.count == b.count
    for f in ("mean", "variance", "std", "norm_l2"):
        torch.testing.assert_close(getattr(a, f), getattr(b, f), rtol=tol, atol=tol)
    assert torch.equal(a.num_nonzeros, b.num_nonzeros)
    assert torch.equal(a.min, b.min)
    assert torch.equal(a.max, b.max)


# --- oracle against a NumPy f64 pin ---

def test_oracle_matches_numpy_pin():
    a = _pin_matrix()
    s, q, mn, mx, nnz = reference.dense_colstats(torch.from_numpy(a))
    assert s.dtype == q.dtype == torch.float64
    assert mn.dtype == mx.dtype == torch.float32 and nnz.dtype == torch.int64
    np.testing.assert_allclose(s.numpy(), a.sum(0), rtol=1e-15, atol=0)
    np.testing.assert_allclose(q.numpy(), (a * a).sum(0), rtol=1e-15, atol=0)
    np.testing.assert_array_equal(mn.numpy(), a.min(0).astype(np.float32))
    np.testing.assert_array_equal(mx.numpy(), a.max(0).astype(np.float32))
    np.testing.assert_array_equal(nnz.numpy(), (a != 0).sum(0))

    summ = column_stats(DenseShard(torch.from_numpy(a), _labels(7)))
    assert summ.count == 7
    np.testing.assert_allclose(summ.mean.numpy(), a.mean(0), rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(summ.variance.numpy(), a.var(0, ddof=1),
                               rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(summ.std.numpy(), a.std(0, ddof=1),
                               rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(summ.norm_l2.numpy(), np.sqrt((a * a).sum(0)),
                               rtol=1e-15, atol=0)
    # zero column and constant column: variance exactly 0
    assert summ.variance[1].item() == 0.0 and summ.variance[2].item() == 0.0
    assert summ.mean.dtype == summ.variance.dtype == summ.std.dtype == torch.float64


def test_single_row_has_zero_variance():
    a = torch.from_numpy(_pin_matrix()[:1].copy())
    summ = column_stats(DenseShard(a, _labels(1)))
    assert summ.count == 1
    assert torch.equal(summ.variance, torch.zeros(5, dtype=torch.float64))
    assert torch.equal(summ.mean, a[0])
    sc = StandardScaler().fit(DenseShard(a, _labels(1)))
    assert torch.equal(sc.scale, torch.ones(5, dtype=torch.float64))


# the shapes and dtypes of the GPU tier (test_gpu_stats.py), on the oracle
SHAPES = [(1, 7), (3, 1), (1037, 1000), (517, 2051), (8192, 1536)]


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32,
                                   torch.float8_e4m3fn, torch.float64],
                         ids=["bf16", "f32", "fp8", "f64"])
def test_ops_dense_colstats_and_scale_on_cpu(dtype, n, d):
    g = torch.Generator().manual_seed(1000 * n + d)
    a = torch.randn(n, d, generator=g) * 3.0
    a[torch.rand(n, d, generator=g) < 0.2] = 0.0
    q = a.to(dtype)
    x = q.to(torch.float64).numpy()
    s, sq, mn, mx, nnz = ops.dense_colstats(q)
    np.testing.assert_allclose(s.numpy(), x.sum(0), rtol=0,
                               atol=1e-12 * max(np.abs(x).sum(0).max(), 1e-300))
    np.testing.assert_allclose(sq.numpy(), (x * x).sum(0), rtol=1e-12, atol=0)
    np.testing.assert_array_equal(mn.numpy(), x.min(0).astype(np.float32))
    np.testing.assert_array_equal(mx.numpy(), x.max(0).astype(np.float32))
    np.testing.assert_array_equal(nnz.numpy(), (x != 0).sum(0))
    scale = torch.linspace(0.5, 2.0, d)
    if dtype == torch.float8_e4m3fn:
        with pytest.raises(NotImplementedError):
            ops.dense_scale_cols(q, scale)
        return
    acc = torch.float64 if dtype == torch.float64 else torch.float32
    want = (q.to(acc) * scale.to(acc)).to(dtype)
    out = ops.dense_scale_cols(q, scale)
    assert out.dtype == dtype and torch.equal(out, want)
    assert ops.dense_scale_cols(q, scale, out=q) is q and torch.equal(q, want)


# --- column_stats across shard kinds ---

def test_column_stats_agrees_across_shard_kinds():
    a = torch.from_numpy(_pin_matrix())
    y = _labels(7)
    ref = column_stats(DenseShard(a, y))
    # bf16: statistics of the bf16-rounded values (exact for this matrix,
    # checked, so one f64 summary serves as the reference for all kinds)
    a16 = a.to(torch.bfloat16)
    assert torch.equal(a16.to(torch.float64), a)
    _assert_summary_close(column_stats(DenseShard(a16, y)), ref)
    _assert_summary_close(column_stats(_to_csr(a, y)), ref)
    _assert_summary_close(column_stats(_to_csr(a, y, deterministic=False)), ref)
    mixed = MixedShard([DenseShard(a[:3].contiguous(), y[:3]),
                        _to_csr(a[3:].contiguous(), y[3:])])
    _assert_summary_close(column_stats(mixed), ref)


def test_bf16_stats_are_those_of_the_rounded_values():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(33, 9, generator=g, dtype=torch.float64) * 3.7
    y = _labels(33)
    a16 = a.to(torch.bfloat16)
    got = column_stats(DenseShard(a16, y))
    want = column_stats(DenseShard(a16.to(torch.float64), y))
    _assert_summary_close(got, want)
    assert not torch.equal(a16.to(torch.float64), a)


def test_csr_zero_folding():
    n = 6
    a = torch.zeros(n, 3, dtype=torch.float64)
    a[:, 0] = torch.tensor([2.0, 3.0, 1.5, 4.0, 2.5, 1.25])  # stored in every row
    a[2, 1] = 5.0                                            # one stored value
    a[4, 2] = -7.0
    summ = column_stats(_to_csr(a, _labels(n)))
    assert summ.min[0].item() == 1.25 > 0
    assert summ.min[1].item() == 0.0 and summ.max[1].item() == 5.0
    assert summ.min[2].item() == -7.0 and summ.max[2].item() == 0.0
    assert summ.num_nonzeros.tolist() == [6, 1, 1]
    # implicit zeros count as samples
    assert summ.mean[1].item() == pytest.approx(5.0 / n, rel=1e-15)
    # an explicitly stored zero is a sample but not a non-zero
    a2 = a.clone()
    a2[0, 0] = 0.0
    s2 = column_stats(_to_csr(a2, _labels(n), dense_cols=(0,)))
    assert s2.num_nonzeros[0].item() == 5 and s2.min[0].item() == 0.0


# --- scale factor and transform ---

def test_scale_factor_and_unit_variance():
    a = torch.from_numpy(_pin_matrix())
    shard = DenseShard(a, _labels(7))
    sc = StandardScaler().fit(shard)
    assert sc.scale[1].item() == 1.0 and sc.scale[2].item() == 1.0  # zero / constant
    torch.testing.assert_close(sc.scale[0], 1.0 / sc.summary.std[0], rtol=1e-15, atol=0)
    out = sc.transform(shard)
    v = column_stats(out).variance
    for c in (0, 3, 4):
        assert abs(v[c].item() - 1.0) <= 1e-12
    assert torch.equal(out.features[:, 2], a[:, 2])  # intercept-like column survives


def test_scale_is_f32_for_low_precision_shards():
    a = torch.from_numpy(_pin_matrix())
    for dt in (torch.float32, torch.bfloat16):
        sc = StandardScaler().fit(DenseShard(a.to(dt), _labels(7)))
        assert sc.scale.dtype == torch.float32
        out = sc.transform(DenseShard(a.to(dt), _labels(7)))
        assert out.features.dtype == dt
        want = (a.to(dt).float() * sc.scale).to(dt)
        assert torch.equal(out.features, want)


def test_transform_out_of_place_and_in_place_dense():
    a = torch.from_numpy(_pin_matrix())
    shard = DenseShard(a.clone(), _labels(7))
    sc = StandardScaler().fit(shard)
    out = sc.transform(shard)
    assert out is not shard and torch.equal(shard.features, a)
    assert out.features.data_ptr() != shard.features.data_ptr()
    same = sc.transform(shard, inplace=True)
    assert same is shard and torch.equal(shard.features, out.features)


def _random_sparse(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, d, generator=g, dtype=torch.float64)
    a = a * (torch.rand(n, d, generator=g) < 0.3)
    a = a * torch.logspace(-2, 2, d, dtype=torch.float64)
    y = (torch.rand(n, generator=g) < 0.5).to(torch.float32)
    return a, y


def test_transform_csr_keeps_csr_and_csc_consistent():
    a, y = _random_sparse(40, 12, seed=5)
    shard = _to_csr(a, y)
    val0, cval0 = shard.val.clone(), shard.csc[2].clone()
    sc = StandardScaler().fit(shard)
    out = sc.transform(shard)
    # source untouched, structure shared, only the value arrays are new
    assert torch.equal(shard.val, val0) and torch.equal(shard.csc[2], cval0)
    assert out.rowptr is shard.rowptr and out.col is shard.col
    assert out.csc[0] is shard.csc[0] and out.csc[1] is shard.csc[1]
    assert out.csc_heavy["cols"] is shard.csc_heavy["cols"]
    assert out.val.data_ptr() != shard.val.data_ptr()
    # rebuilt from scratch from the scaled triplets
    rebuilt = CSRShard(shard.rowptr, shard.col, out.val.clone(), y, shard.d)
    assert torch.equal(out.csc[2], rebuilt.csc[2])
    w = torch.linspace(-1, 1, shard.d, dtype=torch.float64)
    g1, lc1 = out.eval(w, ops.LOSS_LOGISTIC)
    g2, lc2 = rebuilt.eval(w, ops.LOSS_LOGISTIC)
    assert torch.equal(g1, g2) and torch.equal(lc1, lc2)
    # in place: same object, same numbers
    same = sc.transform(shard, inplace=True)
    assert same is shard
    assert torch.equal(shard.val, out.val) and torch.equal(shard.csc[2], out.csc[2])
    # matches the dense transform of the same matrix
    dense = sc.transform(DenseShard(a, y))
    torch.testing.assert_close(column_stats(out).variance,
                               column_stats(dense).variance, rtol=1e-12, atol=1e-12)


def test_transform_mixed_part_by_part():
    a, y = _random_sparse(30, 8, seed=6)
    mixed = MixedShard([DenseShard(a[:10].contiguous(), y[:10]),
                        _to_csr(a[10:].contiguous(), y[10:])])
    sc = StandardScaler().fit(mixed)
    out = sc.transform(mixed)
    assert isinstance(out, MixedShard) and out is not mixed
    want = a * sc.scale
    want_csr = _to_csr(want[10:].contiguous(), y[10:])

    def check(m):
        assert torch.equal(m.parts[0].features, want[:10])
        assert torch.equal(m.parts[1].val, want_csr.val)
        assert torch.equal(m.parts[1].csc[2], want_csr.csc[2])

    check(out)
    assert not torch.equal(mixed.parts[0].features, want[:10])  # source untouched
    assert sc.transform(mixed, inplace=True) is mixed
    check(mixed)


@pytest.mark.parametrize("k", [1, 3])
def test_unscale_weights_margins_identity(k):
    a, y = _random_sparse(25, 7, seed=8)
    shard = DenseShard(a, y)
    sc = StandardScaler().fit(shard)
    out = sc.transform(shard)
    g = torch.Generator().manual_seed(9)
    w = torch.randn(7 * k, generator=g, dtype=torch.float64)
    wu = sc.unscale_weights(w, num_classes=k)
    assert wu.shape == w.shape
    if k == 1:
        m_orig, m_scaled = shard.margins(wu), out.margins(w)
    else:
        m_orig = a @ wu.reshape(7, k)
        m_scaled = out.features @ w.reshape(7, k)
    torch.testing.assert_close(m_orig, m_scaled, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(sc.scale_weights(wu, k), w, rtol=1e-14, atol=0)


# --- trainers ---

def _probe_problem():
    shard, _ = generate_dense_problem(n=2000, d=64, seed=0, dtype=torch.float64)
    sc = torch.logspace(-2, 2, 64, dtype=torch.float64)
    return DenseShard(shard.features * sc, shard.labels)


def test_trainer_feature_scaling_on_ill_scaled_problem():
    raw = _probe_problem()
    feats0 = raw.features.clone()
    kw = dict(num_iterations=20, convergence_tol=0.0)
    base = LogisticRegressionWithAGD.train(raw, **kw)
    off = LogisticRegressionWithAGD.train(raw, feature_scaling=False, **kw)
    assert off.loss_history == base.loss_history  # exact
    assert torch.equal(off.weights, base.weights)

    on = LogisticRegressionWithAGD.train(raw, feature_scaling=True, **kw)
    assert torch.equal(raw.features, feats0)  # out of place
    assert len(on.loss_history) == len(base.loss_history) == 20
    print("loss@20 raw", base.loss_history[-1], "scaled", on.loss_history[-1])
    assert on.loss_history[-1] < 0.5 * base.loss_history[-1]
    # the returned weights live in the ORIGINAL space
    _, lc = raw.eval(on.weights, ops.LOSS_LOGISTIC, need_grad=False)
    loss_raw = float(lc[0] / lc[1])
    assert abs(loss_raw - on.loss_history[-1]) <= 1e-9 * abs(on.loss_history[-1])

    # "inplace" overwrites the caller's shard and gives the same model
    raw2 = DenseShard(feats0.clone(), raw.labels)
    inp = LogisticRegressionWithAGD.train(raw2, feature_scaling="inplace", **kw)
    assert inp.loss_history == on.loss_history
    assert not torch.equal(raw2.features, feats0)
    with pytest.raises(ValueError):
        LogisticRegressionWithAGD.train(raw, feature_scaling="yes", **kw)


def test_trainer_initial_weights_are_original_space():
    raw = _probe_problem()
    kw = dict(num_iterations=3, convergence_tol=0.0)
    first = LogisticRegressionWithAGD.train(raw, feature_scaling=True, **kw)
    # warm start from original-space weights: the first evaluated loss is the
    # loss of those weights, i.e. no worse than where `first` ended
    second = LogisticRegressionWithAGD.train(
        raw, feature_scaling=True, initial_weights=first.weights, **kw)
    assert second.loss_history[0] <= first.loss_history[-1] * (1 + 1e-9)


def test_sgd_trainer_feature_scaling():
    from sparkagd_amd import LogisticRegressionWithSGD

    raw = _probe_problem()
    kw = dict(num_iterations=15, step_size=1.0)
    base = LogisticRegressionWithSGD.train(raw, **kw)
    off = LogisticRegressionWithSGD.train(raw, feature_scaling=False, **kw)
    assert off.loss_history == base.loss_history
    assert torch.equal(off.weights, base.weights)
    on = LogisticRegressionWithSGD.train(raw, feature_scaling=True, **kw)
    # weights come back in the original space: same margins as the scaled
    # weights on the scaled shard
    sc = StandardScaler().fit(raw)
    torch.testing.assert_close(raw.margins(on.weights),
                               sc.transform(raw).margins(sc.scale_weights(on.weights)),
                               rtol=1e-10, atol=1e-10)
    _, lc_on = raw.eval(on.weights, ops.LOSS_LOGISTIC, need_grad=False)
    _, lc_base = raw.eval(base.weights, ops.LOSS_LOGISTIC, need_grad=False)
    assert float(lc_on[0]) < float(lc_base[0])


def test_softmax_trainer_feature_scaling_weights_in_original_space():
    from sparkagd_amd import generate_multiclass_problem

    shard, _ = generate_multiclass_problem(300, 10, 3, seed=2, dtype=torch.float64)
    raw = DenseShard(shard.features * torch.logspace(-1, 1, 10, dtype=torch.float64),
                     shard.labels)
    m = SoftmaxRegressionWithAGD.train(raw, 3, num_iterations=5,
                                       convergence_tol=0.0, feature_scaling=True)
    # softmax loss of the returned weights on the RAW features
    z = raw.features @ m.weights.reshape(10, 3)
    lse = torch.logsumexp(z, dim=1)
    zy = z[torch.arange(300), raw.labels.long()]
    loss = float((lse - zy).mean())
    assert abs(loss - m.loss_history[-1]) <= 1e-9 * abs(loss)


# --- streamed / unsupported ---

def test_streamed_shard_stats_and_unsupported_transforms():
    a, y = _random_sparse(50, 6, seed=11)
    dense = DenseShard(a, y)
    streamed = HostStreamedDenseShard(a, y, device="cpu", chunk_rows=16)
    _assert_summary_close(column_stats(streamed), column_stats(dense))
    sc = StandardScaler().fit(streamed)
    with pytest.raises(NotImplementedError):
        sc.transform(streamed)
    f8 = DenseShard(a.to(torch.float32).to(torch.float8_e4m3fn), y)
    sc8 = StandardScaler().fit(f8)
    assert sc8.scale.dtype == torch.float32
    with pytest.raises(NotImplementedError, match="quantis"):
        sc8.transform(f8)


def test_allreduce_op_keyword():
    c = Communicator()
    t = torch.tensor([1.0, 2.0])
    assert c.allreduce_(t) is t and c.allreduce_(t, op="min") is t
    assert c.allreduce_(t, op="max") is t
    with pytest.raises(ValueError):
        c.allreduce_(t, op="prod")


# --- gloo world size 2 ---

def _dist_worker(rank, world, init_file, out_dir):
    torch.distributed.init_process_group(
        "gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    try:
        a, y = _random_sparse(37, 6, seed=21)
        lo, hi = (0, 11) if rank == 0 else (11, 37)  # uneven split
        part_a, part_y = a[lo:hi].contiguous(), y[lo:hi]
        comm = Communicator()
        dense = column_stats(DenseShard(part_a, part_y), comm)
        sparse = column_stats(_to_csr(part_a, part_y), comm)
        scale = StandardScaler().fit(DenseShard(part_a, part_y), comm).scale
        torch.save({"dense": dense.__dict__, "sparse": sparse.__dict__,
                    "scale": scale}, os.path.join(out_dir, f"r{rank}.pt"))
    finally:
        torch.distributed.destroy_process_group()


def test_two_rank_summaries_identical_and_match_single_process():
    fd, init_file = tempfile.mkstemp(prefix="sparkagd_stats_", suffix=".init")
    os.close(fd)
    os.unlink(init_file)
    with tempfile.TemporaryDirectory() as out_dir:
        mp.spawn(_dist_worker, args=(2, init_file, out_dir), nprocs=2, join=True)
        r0 = torch.load(os.path.join(out_dir, "r0.pt"))
        r1 = torch.load(os.path.join(out_dir, "r1.pt"))
    if os.path.exists(init_file):
        os.unlink(init_file)
    a, y = _random_sparse(37, 6, seed=21)
    single = column_stats(DenseShard(a, y))
    assert torch.equal(r0["scale"], r1["scale"])
    for kind in ("dense", "sparse"):
        s0, s1 = r0[kind], r1[kind]
        assert s0["count"] == s1["count"] == 37
        for f in ("mean", "variance", "std", "num_nonzeros", "min", "max", "norm_l2"):
            assert torch.equal(s0[f], s1[f]), (kind, f)
        _assert_summary_close(ColumnSummary(**s0), single, tol=1e-12)
    assert math.isfinite(float(r0["scale"].sum()))
