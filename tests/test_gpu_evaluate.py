"""HIP metrics kernels (k_binary_metrics, k_multiclass_metrics) against the
plain-torch oracles in ``ops/reference.py``, and ``evaluate`` end to end on
GPU shards of every kind.

Contract. The oracle is fed the same margins the kernel reads (device
produced ones are copied to the CPU):

* histograms, confusions and the NaN count are EXACTLY equal (integer
  accumulation: unweighted examples add 1, weighted ones llrint(w * 2^32));
* each binary f64 sum is within 1e-9 * Σ|w * term| of the oracle (the bound
  ``tests/test_gpu_stats.py`` gives f64 moment sums); a sum the oracle finds
  non-finite (±inf margins) must be the same non-finite value;
* the multiclass loss sum is within rtol 1e-5 (f32 per-row loss with the
  fast exp, the tolerance ``tests/test_gpu_kernels.py`` gives the softmax
  loss sum);
* two calls are bitwise equal, and a call on a side stream equals both.
"""

import functools
import math

import pytest
import torch

from sparkagd_amd import (
    CSRShard,
    DenseShard,
    HostStreamedDenseShard,
    LinearModel,
    LogisticRegressionWithAGD,
    SoftmaxRegressionWithAGD,
    evaluate,
    ops,
)
from sparkagd_amd.data import (
    generate_csr_problem,
    generate_dense_problem,
    generate_multiclass_problem,
)
from sparkagd_amd.evaluation import _edges_for
from sparkagd_amd.ops import multiclass as mc
from sparkagd_amd.ops import reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# a single row; just under a wave; just over a block; many blocks + ragged tail
BIN_N = [1, 63, 257, 100003]
# no edges; one edge; the default; the LDS-resident maximum (second template)
BIN_B = [1, 2, 1000, 4096]
CUT = 0.7


@functools.lru_cache(maxsize=None)
def _binary_case(n, nbins, weighted, dtype):
    """CPU inputs, built once: margins = randn * 4 with exact edge values,
    the cut itself, ±0.0 and ±inf planted; a finite twin (infs -> ±50) for
    the sums; the oracle's answers for both."""
    g = torch.Generator().manual_seed(7919 * n + nbins + (1 if weighted else 0))
    edges = _edges_for(nbins, None, dtype)
    z = (torch.randn(n, generator=g, dtype=torch.float64) * 4).to(dtype)
    special = [0.0, -0.0, math.inf, -math.inf, CUT]
    if nbins > 1:
        picks = {0, (nbins - 2) // 2, nbins - 2}
        special += [float(edges[j]) for j in sorted(picks)]
        special += [float(torch.nextafter(edges[0], edges[0] - 1))]
    for j, v in enumerate(special):
        if n > 4 * len(special):
            z[(j * 37 + 5) % n] = v
            z[(j * 53 + 11 + n // 2) % n] = v
    if n == 1:
        z[0] = float(edges[0]) if nbins > 1 else 0.0
    y = (torch.rand(n, generator=g) < 0.4).to(torch.float32)
    w = None
    if weighted:
        w = torch.rand(n, generator=g) * 4
        w[torch.rand(n, generator=g) < 0.1] = 0.0
    z_fin = torch.where(torch.isinf(z), torch.sign(z) * 50, z)
    ref = reference.binary_metrics(z, y, edges, CUT, w)
    ref_fin = reference.binary_metrics(z_fin, y, edges, CUT, w)
    # Σ|w * term| of the finite twin, the scale of the sums' bound
    zd, yd = z_fin.double(), y.double()
    wd = torch.ones(n, dtype=torch.float64) if w is None else w.double()
    ls = torch.where(yd > 0.5, reference.stable_softplus(-zd),
                     reference.stable_softplus(zd))
    diff = zd - yd
    scale = torch.stack([t.abs().sum() for t in (
        wd, wd * ls, wd * diff * diff, wd * diff.abs(), wd * yd,
        wd * yd * yd, wd * diff)])
    return z, z_fin, y, w, edges, ref, ref_fin, scale


def _run_binary(z, y, edges, w):
    out = ops.binary_metrics(z.to(DEV), y.to(DEV), edges, CUT,
                             None if w is None else w.to(DEV))
    return [t.cpu() for t in out]


def _assert_ints_equal(got, ref):
    for name, a, b in zip(("hist_pos", "hist_neg", "conf"), got[:3], ref[:3]):
        assert a.dtype == torch.int64 and a.shape == b.shape, name
        assert torch.equal(a, b), (name, (a - b).abs().max().item())
    assert int(got[4]) == int(ref[4])


def _bitwise_equal(a, b):
    return all(torch.equal(x.reshape(-1).view(torch.int64) if x.dtype == torch.float64
                           else x.reshape(-1), y.reshape(-1).view(torch.int64)
                           if y.dtype == torch.float64 else y.reshape(-1))
               for x, y in zip(a[:5], b[:5]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("nbins", BIN_B)
@pytest.mark.parametrize("n", BIN_N)
def test_binary_metrics_match_oracle(n, nbins, weighted, dtype):
    z, z_fin, y, w, edges, ref, ref_fin, scale = _binary_case(n, nbins, weighted, dtype)
    got = _run_binary(z, y, edges, w)
    _assert_ints_equal(got, ref)
    assert int(got[0].sum() + got[1].sum()) == int(ref[0].sum() + ref[1].sum())
    assert got[3].dtype == torch.float64 and got[3].shape == (7,)
    finite = torch.isfinite(ref[3])
    bad = ~finite
    assert torch.equal(torch.isnan(got[3][bad]), torch.isnan(ref[3][bad]))
    inf = bad & ~torch.isnan(ref[3])
    assert torch.equal(got[3][inf], ref[3][inf])
    if weighted:
        assert float(got[5]) == float(ref[5])
    else:
        assert float(got[5]) == math.inf

    got_fin = _run_binary(z_fin, y, edges, w)
    _assert_ints_equal(got_fin, ref_fin)
    err = (got_fin[3] - ref_fin[3]).abs()
    print("sum err / bound:", (err / (1e-9 * scale + 1e-300)).tolist())
    assert bool((err <= 1e-9 * scale).all()), (err, scale)

    again = _run_binary(z, y, edges, w)
    assert _bitwise_equal(got, again)


def test_binary_metrics_on_side_stream():
    z, _, y, w, edges, ref, _, _ = _binary_case(100003, 1000, True, torch.float32)
    base = _run_binary(z, y, edges, w)
    zd, yd, wd = z.to(DEV), y.to(DEV), w.to(DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        out = ops.binary_metrics(zd, yd, edges, CUT, wd)
    side.synchronize()
    out = [t.cpu() for t in out]
    _assert_ints_equal(out, ref)
    assert _bitwise_equal(out, base)


def test_binary_metrics_counts_nan_margins():
    z, _, y, w, edges, _, _, _ = _binary_case(257, 1000, True, torch.float32)
    z = z.clone()
    z[[3, 100, 256]] = math.nan
    ref = reference.binary_metrics(z, y, edges, CUT, w)
    got = _run_binary(z, y, edges, w)
    _assert_ints_equal(got, ref)
    assert int(got[4]) == 3


# --- multiclass ---

# smallest; not a multiple of 4; a template size; just past the template
# sizes (wave-per-row, LDS confusion); large K (global confusion)
MULTI = [(k, n) for k in (2, 3, 16, 33) for n in (1, 65, 4099)] + [(1000, 257)]


@functools.lru_cache(maxsize=None)
def _multi_case(k, n, weighted):
    g = torch.Generator().manual_seed(104729 * k + n)
    kc = mc.padded_k(k)
    z = torch.full((n, kc), 1.0e9)  # pad columns must never be read as classes
    z[:, :k] = torch.randn(n, k, generator=g) * 3
    top2 = z[:, :k].topk(2, dim=1).values
    assert bool((top2[:, 0] > top2[:, 1]).all()), "case must have no row ties"
    y = torch.randint(0, k, (n,), generator=g).to(torch.float32)
    w = None
    if weighted:
        w = torch.rand(n, generator=g) * 4
        w[torch.rand(n, generator=g) < 0.1] = 0.0
    zf = z.reshape(-1).contiguous()
    return zf, y, w, kc, reference.multiclass_metrics(zf, y, k, kc, w)


def _run_multi(zf, y, k, w):
    out = mc.multiclass_metrics(zf.to(DEV), y.to(DEV), k,
                                None if w is None else w.to(DEV))
    return [t.cpu() for t in out]


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("k,n", MULTI)
def test_multiclass_metrics_match_oracle(k, n, weighted):
    zf, y, w, kc, ref = _multi_case(k, n, weighted)
    got = _run_multi(zf, y, k, w)
    assert got[0].dtype == torch.int64 and got[0].shape == (k, k)
    assert torch.equal(got[0], ref[0])
    assert int(got[2]) == 0
    print("sums", got[1].tolist(), ref[1].tolist())
    assert abs(float(got[1][0] - ref[1][0])) <= 1e-9 * abs(float(ref[1][0]))
    torch.testing.assert_close(got[1][1], ref[1][1], rtol=1e-5, atol=0.0)
    again = _run_multi(zf, y, k, w)
    assert torch.equal(got[0], again[0])
    assert torch.equal(got[1].view(torch.int64), again[1].view(torch.int64))


@pytest.mark.parametrize("k", [7, 40, 200])
def test_multiclass_ties_pick_lowest_index(k):
    """Rows full of exact ties (margins drawn from {0, 1, 2}), thread-per-row
    (k=7) and wave-per-row with ties across lanes (40) and across a lane's
    own strided classes (200); the oracle is an explicit first-maximum loop."""
    n = 61
    g = torch.Generator().manual_seed(k)
    kc = mc.padded_k(k)
    z = torch.full((n, kc), 5.0)
    z[:, :k] = torch.randint(0, 3, (n, k), generator=g).to(torch.float32)
    z[0, :k] = 1.0   # every class tied
    z[1, :k] = 0.0
    z[1, k - 1] = 2.0  # unique maximum in the last class
    y = torch.randint(0, k, (n,), generator=g).to(torch.float32)
    conf = torch.zeros(k, k, dtype=torch.int64)
    for i in range(n):
        best, arg = -math.inf, 0
        for c in range(k):
            if float(z[i, c]) > best:
                best, arg = float(z[i, c]), c
        conf[int(y[i]), arg] += 1
    got = _run_multi(z.reshape(-1).contiguous(), y, k, None)
    assert torch.equal(got[0], conf)
    ref = reference.multiclass_metrics(z.reshape(-1), y, k, kc, None)
    assert torch.equal(ref[0], conf)


# --- end to end ---

def _cpu_model(model):
    if hasattr(model, "num_classes"):
        return type(model)(model.weights.cpu(), model.loss_history, model.num_classes)
    return LinearModel(model.weights.cpu(), model.loss_history, model.link)


def _dense_cpu(shard):
    return DenseShard(shard.features.cpu(), shard.labels.cpu(),
                      None if shard.sample_weight is None else shard.sample_weight.cpu())


def _csr_cpu(shard):
    return CSRShard(shard.rowptr.cpu(), shard.col.cpu(), shard.val.cpu(),
                    shard.labels.cpu(), shard.d, deterministic=False,
                    sample_weight=None if shard.sample_weight is None
                    else shard.sample_weight.cpu())


def _assert_binary_equal(gpu, cpu):
    assert torch.equal(gpu.hist_pos, cpu.hist_pos)
    assert torch.equal(gpu.hist_neg, cpu.hist_neg)
    assert gpu.confusion == cpu.confusion
    assert gpu.count == cpu.count
    assert abs(gpu.log_loss - cpu.log_loss) <= 1e-9 * abs(cpu.log_loss)
    assert gpu.area_under_roc == cpu.area_under_roc


def test_evaluate_dense_bf16_end_to_end():
    n, d = 4096, 256
    shard, _ = generate_dense_problem(n=n, d=d, seed=3, device=DEV, dtype=torch.bfloat16)
    model = LogisticRegressionWithAGD.train(shard, num_iterations=10)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    z = model.score(shard)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(DEV) - base
    print("score(): extra bytes", extra, "of n*d", n * d)
    assert extra < n * d  # no f32 (4*n*d) or even bf16 (2*n*d) feature copy
    assert z.shape == (n,) and z.dtype == torch.float32
    pred = model.predict_shard(shard)
    assert torch.equal(pred, (z > 0).to(torch.float32))
    gpu = evaluate(model, shard)
    cpu = evaluate(_cpu_model(model), _dense_cpu(shard), margins=z.cpu())
    _assert_binary_equal(gpu, cpu)
    assert gpu.area_under_roc > 0.8
    assert abs(gpu.accuracy - float((pred == shard.labels).double().mean())) < 1e-12


def test_evaluate_csr_end_to_end():
    shard, _ = generate_csr_problem(n=4096, d=2000, nnz_per_row=20, seed=4, device=DEV)
    g = torch.Generator().manual_seed(0)
    shard.sample_weight = (torch.rand(4096, generator=g) * 3).to(DEV)
    model = LogisticRegressionWithAGD.train(shard, num_iterations=10)
    z = model.score(shard)
    gpu = evaluate(model, shard, num_bins=200, threshold=0.3)
    cpu = evaluate(_cpu_model(model), _csr_cpu(shard), num_bins=200,
                   threshold=0.3, margins=z.cpu())
    _assert_binary_equal(gpu, cpu)
    assert gpu.area_under_roc > 0.8


def test_evaluate_softmax_end_to_end():
    k = 5
    shard, _ = generate_multiclass_problem(n=4096, d=64, num_classes=k, seed=5,
                                           device=DEV, dtype=torch.bfloat16)
    model = SoftmaxRegressionWithAGD.train(shard, k, num_iterations=10)
    z = model.score(shard)
    assert z.shape == (4096, k)
    gpu = evaluate(model, shard)
    cpu = evaluate(_cpu_model(model), _dense_cpu(shard), margins=z.cpu())
    assert torch.equal(gpu.confusion, cpu.confusion)
    assert abs(gpu.log_loss - cpu.log_loss) <= 1e-5 * cpu.log_loss
    assert gpu.accuracy == cpu.accuracy and gpu.accuracy > 0.5
    assert torch.equal(model.predict_shard(shard).cpu(),
                       reference.argmax_lowest(z.cpu()).to(torch.float32))


def test_evaluate_fp8_and_host_streamed_shards():
    n, d = 3001, 128
    g = torch.Generator().manual_seed(6)
    a = torch.randn(n, d, generator=g)
    w = torch.randn(d, generator=g) / math.sqrt(d)
    y = (a @ w + 0.1 * torch.randn(n, generator=g) > 0).to(torch.float32)
    model = LinearModel(w.to(DEV), [], "logistic")
    fp8 = DenseShard(a.to(torch.float8_e4m3fn).to(DEV), y.to(DEV))
    streamed = HostStreamedDenseShard(a.to(torch.bfloat16).pin_memory(), y,
                                      device=DEV, chunk_rows=1024)
    assert streamed.features_host.is_pinned() and not streamed.features_host.is_cuda
    for shard in (fp8, streamed):
        z = model.score(shard)
        gpu = evaluate(model, shard, num_bins=64)
        cpu = evaluate(_cpu_model(model), DenseShard(a, y), num_bins=64,
                       margins=z.cpu())
        _assert_binary_equal(gpu, cpu)
        assert gpu.area_under_roc > 0.8
