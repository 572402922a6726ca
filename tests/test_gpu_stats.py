"""HIP column-statistics and column-scaling kernels against the CPU f64
oracle, plus the feature-scaled trainer end to end on the GPU.

Accuracy contract for the moments (f64 accumulation, n <= 1e5), checked on
the SAME quantised values the kernel reads:

    |sum - ref|      <= 1e-9 * sum|a|
    |sumsq - ref|    <= 1e-9 * ref
    |variance - ref| <= 1e-9 * (sumsq_ref / n)
    min, max, nnz exact; two calls bitwise equal.
"""

import functools

import pytest
import torch

from sparkagd_amd import (
    CSRShard,
    DenseShard,
    LogisticRegressionWithAGD,
    StandardScaler,
    column_stats,
    ops,
)
from sparkagd_amd.data import generate_csr_problem, generate_dense_problem
from sparkagd_amd.ops import reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (1, 7) / (3, 1): single row / single column, scalar-load path;
# (1037, 1000): d a multiple of the bf16 and f32 vector widths but not fp8's;
# (517, 2051): unaligned d (scalar path), a partial last column slab, rows
#   that do not divide evenly into row blocks;
# (8192, 1536): 16-B path for every dtype, 4096 row blocks of 2 rows (fp8,
#   bf16) / 2 column slabs x 2048 row blocks (f32); 48 MB at f32.
SHAPES = [(1, 7), (3, 1), (1037, 1000), (517, 2051), (8192, 1536)]
STAT_DTYPES = [torch.bfloat16, torch.float32, torch.float8_e4m3fn]


@functools.lru_cache(maxsize=None)
def _dense_case(dtype, n, d):
    """(quantised CPU matrix, its f64 oracle moments, sum|a|) — built once."""
    g = torch.Generator().manual_seed(1000 * n + d)
    a = torch.randn(n, d, generator=g) * 3.0
    a = a * torch.logspace(-1, 1, d)[None, :].clamp(max=30.0)
    a[torch.rand(n, d, generator=g) < 0.2] = 0.0
    if d > 4 and n > 2:
        a[:, 3] = 0.0   # all-zero column
        a[:, 4] = 1.5   # constant column
    q = a.to(dtype).contiguous()
    ref = reference.dense_colstats(q)
    sabs = q.to(torch.float64).abs().sum(dim=0)
    return q, ref, sabs


def _check_moments(got, ref, sabs):
    s, q, mn, mx, nnz = [t.cpu() for t in got]
    rs, rq, rmn, rmx, rnnz = ref
    assert s.dtype == q.dtype == torch.float64
    assert mn.dtype == mx.dtype == torch.float32 and nnz.dtype == torch.int64
    err_s = ((s - rs).abs() - 1e-9 * sabs).max().item()
    err_q = ((q - rq).abs() - 1e-9 * rq).max().item()
    print(f"max sum err/bound {((s - rs).abs() / (1e-9 * sabs + 1e-300)).max().item():.3g} "
          f"sumsq {((q - rq).abs() / (1e-9 * rq + 1e-300)).max().item():.3g}")
    assert err_s <= 0.0, err_s
    assert err_q <= 0.0, err_q
    assert torch.equal(mn, rmn) and torch.equal(mx, rmx)
    assert torch.equal(nnz, rnnz)


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("dtype", STAT_DTYPES, ids=["bf16", "f32", "fp8"])
def test_dense_colstats_matches_oracle(dtype, n, d):
    from sparkagd_amd.ops import hiplib

    a_cpu, ref, sabs = _dense_case(dtype, n, d)
    a = a_cpu.to(DEV)
    got = ops.dense_colstats(a)
    _check_moments(got, ref, sabs)
    again = ops.dense_colstats(a)
    for x, y in zip(got, again):
        assert torch.equal(x, y)
    # variance through the public API
    y0 = torch.zeros(n)
    v_gpu = column_stats(DenseShard(a, y0.to(DEV))).variance.cpu()
    if dtype == torch.float8_e4m3fn:
        v_ref = column_stats(DenseShard(a_cpu.to(torch.float64), y0)).variance
    else:
        v_ref = column_stats(DenseShard(a_cpu, y0)).variance
    assert ((v_gpu - v_ref).abs() <= 1e-9 * (ref[1] / n)).all()
    if (n, d) == SHAPES[-1]:
        code = hiplib._DTYPE_CODE[dtype]
        assert hiplib.load().agd_dense_rowblocks(n, d, code) > 1


def test_streamed_shard_stats_gpu():
    """Per-chunk moments through the double-buffered chunk loop (5 chunks,
    the last one short) meet the same contract as the resident shard."""
    from sparkagd_amd import HostStreamedDenseShard

    a_cpu, ref, sabs = _dense_case(torch.bfloat16, 1037, 1000)
    y = torch.zeros(1037)
    streamed = HostStreamedDenseShard(a_cpu, y, device=DEV, chunk_rows=256)
    s = column_stats(streamed)
    r = column_stats(DenseShard(a_cpu, y))
    assert s.count == 1037
    assert ((s.mean.cpu() * 1037 - ref[0]).abs() <= 1e-9 * sabs + 1e-300).all()
    assert ((s.variance.cpu() - r.variance).abs() <= 1e-9 * (ref[1] / 1037)).all()
    assert torch.equal(s.min.cpu(), r.min) and torch.equal(s.max.cpu(), r.max)
    assert torch.equal(s.num_nonzeros.cpu(), r.num_nonzeros)
    with pytest.raises(NotImplementedError):
        StandardScaler().fit(streamed).transform(streamed)


def test_dense_colstats_f64_shard():
    a_cpu, _, _ = _dense_case(torch.float32, 517, 2051)
    a64 = a_cpu.to(torch.float64) * 1.000000123  # not representable in f32
    ref = reference.dense_colstats(a64)
    got = ops.dense_colstats(a64.to(DEV))
    _check_moments(got, ref, a64.abs().sum(dim=0))


# --- CSR ---

def _skewed_csr(n, d, nnz_per_row, seed, device, deterministic=True):
    """Zipf-column CSR shard with one column forced empty, one stored in
    every row, and a few explicitly stored zeros. Built on CPU, moved."""
    src, _ = generate_csr_problem(n=n, d=d, nnz_per_row=nnz_per_row, seed=seed,
                                  col_dist="zipf")
    col = src.col.clone()
    val = src.val.clone()
    counts = torch.bincount(col.to(torch.int64), minlength=d)
    empty_c = int(torch.argmax(counts))          # the hottest column, emptied
    full_c = (empty_c + 7) % d
    col[col == empty_c] = (empty_c + 1) % d
    col[src.rowptr[:-1].to(torch.int64)] = full_c  # first entry of every row
    val[::97] = 0.0
    return (CSRShard(src.rowptr.to(device), col.to(device), val.to(device),
                     src.labels.to(device), d, deterministic=deterministic),
            empty_c, full_c)


@pytest.fixture
def small_heavy(monkeypatch):
    monkeypatch.setattr(CSRShard, "CSC_HEAVY_T", 48)
    monkeypatch.setattr(CSRShard, "CSC_TASK_S", 32)


def test_csr_colstats_matches_oracle(small_heavy):
    n, d = 3000, 5000
    gpu, empty_c, full_c = _skewed_csr(n, d, 16, 5, DEV)
    cpu, _, _ = _skewed_csr(n, d, 16, 5, "cpu")
    heavy = gpu.csc_heavy
    assert heavy["cols"].numel() > 3, "several columns must be heavy"
    ntasks = torch.diff(heavy["taskptr"])
    assert int(ntasks.max()) > 64, "a combine longer than one wave of tasks"
    assert int((ntasks > 1).sum()) > 3

    ref = reference.csr_colstats(cpu.csc, n, d)
    sabs = reference.csr_colstats((cpu.csc[0], cpu.csc[1], cpu.csc[2].abs()), n, d)[0]
    got = ops.csr_colstats(gpu.csc, n, d, gpu.csc_heavy)
    _check_moments(got, ref, sabs)
    again = ops.csr_colstats(gpu.csc, n, d, gpu.csc_heavy)
    for x, y in zip(got, again):
        assert torch.equal(x, y)
    # no heavy structure: plain thread-per-column pass, same contract
    _check_moments(ops.csr_colstats(gpu.csc, n, d, None), ref, sabs)

    s_gpu, s_cpu = column_stats(gpu), column_stats(cpu)
    assert s_gpu.count == n
    assert ((s_gpu.variance.cpu() - s_cpu.variance).abs()
            <= 1e-9 * (ref[1] / n)).all()
    assert torch.equal(s_gpu.min.cpu(), s_cpu.min)
    assert torch.equal(s_gpu.max.cpu(), s_cpu.max)
    assert torch.equal(s_gpu.num_nonzeros.cpu(), s_cpu.num_nonzeros)
    # empty column: all zeros; full column: stored everywhere, no folded zero
    assert s_gpu.num_nonzeros[empty_c].item() == 0
    assert s_gpu.min[empty_c].item() == 0.0 == s_gpu.max[empty_c].item()
    assert s_gpu.variance[empty_c].item() == 0.0
    stored_full = torch.diff(gpu.csc[0])[full_c].item()
    assert stored_full >= n

    # a shard without a CSC copy builds a temporary one: same bits
    nd, _, _ = _skewed_csr(n, d, 16, 5, DEV, deterministic=False)
    assert nd.csc is None
    s_nd = column_stats(nd)
    assert nd.csc is None
    for f in ("mean", "variance", "min", "max", "num_nonzeros", "norm_l2"):
        assert torch.equal(getattr(s_nd, f), getattr(s_gpu, f)), f


# --- scale kernels ---

@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "f32"])
def test_dense_scale_cols_bit_exact(dtype, n, d):
    a_cpu, _, _ = _dense_case(dtype, n, d)
    g = torch.Generator().manual_seed(d)
    s = torch.exp(torch.randn(d, generator=g) * 2.0)
    want = (a_cpu.float() * s).to(dtype)
    a = a_cpu.to(DEV)
    out = ops.dense_scale_cols(a, s.to(DEV))
    assert out.dtype == dtype and out.data_ptr() != a.data_ptr()
    assert torch.equal(a.cpu().view(torch.uint8), a_cpu.view(torch.uint8))
    assert torch.equal(out.cpu(), want)
    same = ops.dense_scale_cols(a, s.to(DEV), out=a)
    assert same is a and torch.equal(a.cpu(), want)


def test_dense_scale_cols_f64_and_fp8():
    a_cpu, _, _ = _dense_case(torch.float32, 517, 2051)
    a64 = a_cpu.to(torch.float64)
    s = torch.linspace(0.5, 3.0, 2051, dtype=torch.float64)
    out = ops.dense_scale_cols(a64.to(DEV), s.to(DEV))
    assert torch.equal(out.cpu(), a64 * s)
    a8, _, _ = _dense_case(torch.float8_e4m3fn, 1037, 1000)
    with pytest.raises(NotImplementedError):
        ops.dense_scale_cols(a8.to(DEV), torch.ones(1000, device=DEV))


def test_csr_and_csc_scale_vals_bit_exact(small_heavy):
    # 2999 rows x 15 entries: the entry count is odd, so the 4-entry groups
    # of the CSC kernel end in a partial group
    n, d = 2999, 5000
    gpu, empty_c, _ = _skewed_csr(n, d, 15, 6, DEV)
    assert gpu.nnz % 4 != 0
    g = torch.Generator().manual_seed(4)
    s = torch.exp(torch.randn(d, generator=g) * 2.0)
    col, val = gpu.col.cpu(), gpu.val.cpu()
    colptr, _, cval = [t.cpu() for t in gpu.csc]
    want_val = val * s[col.long()]
    want_cval = cval * s[reference._csc_cols(colptr)]

    out_v = ops.csr_scale_vals(gpu.col, gpu.val, s.to(DEV))
    out_c = ops.csc_scale_vals(gpu.csc[0], gpu.csc[2], s.to(DEV),
                               csc_heavy=gpu.csc_heavy)
    assert torch.equal(gpu.val.cpu(), val) and torch.equal(gpu.csc[2].cpu(), cval)
    assert torch.equal(out_v.cpu(), want_val)
    assert torch.equal(out_c.cpu(), want_cval)
    # in place
    v2, c2 = gpu.val.clone(), gpu.csc[2].clone()
    assert ops.csr_scale_vals(gpu.col, v2, s.to(DEV), out=v2) is v2
    assert ops.csc_scale_vals(gpu.csc[0], c2, s.to(DEV), out=c2) is c2
    assert torch.equal(v2.cpu(), want_val) and torch.equal(c2.cpu(), want_cval)


def test_csr_inplace_transform_then_eval_matches_oracle(small_heavy):
    n, d = 3000, 5000
    gpu, _, _ = _skewed_csr(n, d, 16, 5, DEV)
    cpu, _, _ = _skewed_csr(n, d, 16, 5, "cpu")
    sc = StandardScaler().fit(gpu)
    assert sc.scale.dtype == torch.float32 and sc.scale.device.type == "cuda"
    scaled_val = cpu.val * sc.scale.cpu()[cpu.col.long()]
    same = sc.transform(gpu, inplace=True)
    assert same is gpu and torch.equal(gpu.val.cpu(), scaled_val)

    g = torch.Generator().manual_seed(2)
    w = torch.randn(d, generator=g) * 0.01
    grad_h, lc_h = gpu.eval(w.to(DEV), ops.LOSS_LOGISTIC)
    grad_r, lc_r = reference.csr_eval(cpu.rowptr, cpu.col, scaled_val,
                                      cpu.labels, w, ops.LOSS_LOGISTIC, d=d)
    # tolerances of test_gpu_kernels.py::test_csr_eval_matches_reference
    torch.testing.assert_close(grad_h.cpu(), grad_r, rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(lc_h.cpu(), lc_r, rtol=1e-5, atol=1e-6)
    # CSR margins and the CSC gradient saw the same matrix: an out-of-place
    # transform of a fresh shard rebuilt from the scaled triplets agrees bitwise
    rebuilt = CSRShard(gpu.rowptr, gpu.col, gpu.val.clone(), gpu.labels, d)
    assert torch.equal(rebuilt.csc[2], gpu.csc[2])


# --- end to end ---

def test_trainer_feature_scaling_bf16_gpu():
    shard, _ = generate_dense_problem(n=2000, d=64, seed=0, dtype=torch.float64)
    feats = (shard.features * torch.logspace(-2, 2, 64, dtype=torch.float64))
    raw = DenseShard(feats.to(DEV, torch.bfloat16), shard.labels.to(DEV))
    before = raw.features.clone()
    kw = dict(num_iterations=20, convergence_tol=0.0)
    base = LogisticRegressionWithAGD.train(raw, **kw)
    on = LogisticRegressionWithAGD.train(raw, feature_scaling=True, **kw)
    assert torch.equal(raw.features, before)
    print("loss@20 raw", base.loss_history[-1], "scaled", on.loss_history[-1])
    assert on.loss_history[-1] < 0.5 * base.loss_history[-1]

    # margins identity: original shard with mapped-back weights vs the
    # transformed shard with scaled-space weights. The transformed features
    # are re-rounded to bf16 (2^-9 relative per element), so the identity
    # holds at mixed-precision level relative to the norm — the criterion
    # and the 1e-2 bound of test_gpu_optimizer.py lines 226-228.
    sc = StandardScaler().fit(raw)
    scaled = sc.transform(raw)
    assert scaled.features.dtype == torch.bfloat16
    w_scaled = sc.scale_weights(on.weights)
    m_orig = raw.margins(sc.unscale_weights(w_scaled)).double()
    m_scaled = scaled.margins(w_scaled).double()
    num = float(torch.norm(m_orig - m_scaled))
    den = float(torch.norm(m_scaled)) + 1e-30
    print("margins identity rel err", num / den)
    assert num / den < 1e-2, (num, den)
