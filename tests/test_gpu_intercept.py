"""Native intercept on the GPU: the n-space HIP kernels against their
oracles, InterceptShard on every shard kind against the CPU f64 oracle on the
ones-appended data, end-to-end training, and the host-traffic contract."""

import math

import pytest
import torch

from sparkagd_amd import (
    CSRShard,
    DenseShard,
    FreeTailUpdater,
    InterceptShard,
    LogisticGradient,
    LogisticRegressionWithAGD,
    MixedShard,
    SquaredL2Updater,
    ops,
    run,
)
from sparkagd_amd.data import generate_csr_problem, generate_dense_problem
from conftest import assert_rel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
LOSSES = [ops.LOSS_LOGISTIC, ops.LOSS_LEAST_SQUARES, ops.LOSS_HINGE,
          ops.LOSS_SMOOTH_HINGE]
KINDS = [ops.PROX_SIMPLE, ops.PROX_L1, ops.PROX_SQUARED_L2,
         ops.PROX_ELASTIC_NET]


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


# --- 1. multiplier_loss_sum --------------------------------------------------

# 2 097 409 = 8192 * 256 + 257: the grid is capped at 8192 blocks, so the
# grid-stride loop takes a second trip
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2_097_409])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_multiplier_loss_sum(n, dtype):
    from sparkagd_amd.ops import hiplib

    g = _gen(n % 1000 + 1)
    z = torch.randn(n, generator=g, device=DEV, dtype=dtype) * 2.0
    y = (torch.rand(n, generator=g, device=DEV) < 0.7).to(torch.float32)
    mask = (torch.rand(n, generator=g, device=DEV) < 0.6).to(torch.uint8)
    sw = torch.rand(n, generator=g, device=DEV) * 2.0
    feats = torch.empty((n, 1), dtype=dtype, device=DEV)  # shape/dtype carrier
    for loss_type in LOSSES:
        for m, w in ((mask, None), (None, sw), (mask, sw), (None, None)):
            mult, out = hiplib.multiplier_loss_sum(z, y, loss_type, m, w)
            mult0, lc0 = hiplib.dense_multiplier_loss(feats, z, y, loss_type, m, w)
            assert out.shape == (3,) and out.dtype == F64
            assert torch.equal(mult, mult0)
            torch.testing.assert_close(out[:2], lc0, rtol=1e-12, atol=0)
            md = mult.double()
            assert abs(float(out[2] - md.sum())) <= 1e-12 * float(md.abs().sum())
            if m is not None:
                assert float(mult[m == 0].abs().sum()) == 0.0


# --- 2. add_bias_ -------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_add_bias(n, dtype):
    g = _gen(n)
    z = torch.randn(n, generator=g, device=DEV, dtype=dtype)
    src = torch.randn(7, generator=g, device=DEV, dtype=dtype)
    for idx in (0, 6):
        want = z + src[idx]
        got = z.clone()
        ret = ops.add_bias_(got, 1.0, src, idx)
        assert ret is got
        assert torch.equal(got, want)
    got = ops.add_bias_(z.clone(), -0.5, src, 3)
    torch.testing.assert_close(got, z - 0.5 * src[3])
    with pytest.raises(IndexError):
        ops.add_bias_(z.clone(), 1.0, src, 7)
    with pytest.raises(TypeError):
        ops.add_bias_(z.clone(), 1.0, src.to(
            torch.float64 if dtype == torch.float32 else torch.float32), 0)


# --- 3. prox(n_free=1) ----------------------------------------------------------

# 1025 = 4*256 + 1 and 1026 = 2*513: the free coordinate sits in the scalar
# tail for one of f32 (VE=4) / f64 (VE=2) and in the vector body for the
# other, past the first block's first trip
@pytest.mark.parametrize("n", [2, 4, 5, 8, 1025, 1026])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_prox_free_tail(kind, dtype, n):
    from sparkagd_amd.ops import reference

    g = _gen(4)
    w = torch.randn(n, generator=g, device=DEV, dtype=dtype)
    gr = torch.randn(n, generator=g, device=DEV, dtype=dtype)
    lam2 = 0.11 if kind == ops.PROX_ELASTIC_NET else 0.0
    out, reg = ops.prox(kind, w, gr, 0.37, 0.21, lam2, n_free=1)
    out_r, reg_r = reference.prox_free(kind, w.double().cpu(), gr.double().cpu(),
                                       0.37, 0.21, lam2, 1)
    assert out.dtype == dtype and out.shape == (n,)
    torch.testing.assert_close(out.double().cpu(), out_r, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(reg.cpu(), reg_r, rtol=5e-6, atol=5e-6)
    # the head is the plain prox of the head. Not bit for bit: an element
    # that sits in the 16-byte body of one call can sit in the scalar tail of
    # the other, and the two are contracted to fma differently (1 ulp)
    head, reg_h = ops.prox(kind, w[:n - 1].contiguous(), gr[:n - 1].contiguous(),
                           0.37, 0.21, lam2)
    ulp = 4 * torch.finfo(dtype).eps
    torch.testing.assert_close(out[:n - 1], head, rtol=ulp, atol=ulp)
    torch.testing.assert_close(reg, reg_h, rtol=10 * ulp, atol=10 * ulp)


# --- 4. at_margin_update with offset ----------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 4, 5, 4099])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_at_margin_update_offset(n, dtype):
    from sparkagd_amd.ops import hiplib

    g = _gen(n + 7)
    zm, xm, gm = (torch.randn(n, generator=g, device=DEV, dtype=dtype)
                  for _ in range(3))
    src = torch.randn(9, generator=g, device=DEV, dtype=dtype)
    pz, pg, th, c, idx = 0.93, -0.41, 0.37, 0.07, 8
    zn, xn = ops.at_margin_update(zm, xm, gm, pz, pg, th, offset=(c, src, idx))
    zr = pz * zm.double() + pg * gm.double() + c * src[idx].double()
    xr = (1.0 - th) * xm.double() + th * zr
    # inputs are O(1), so the absolute floor equals the relative bound
    tol = 1e-6 if dtype == torch.float32 else 1e-12
    assert zn.dtype == dtype and xn.dtype == dtype
    torch.testing.assert_close(zn.double(), zr, rtol=tol, atol=tol)
    torch.testing.assert_close(xn.double(), xr, rtol=tol, atol=tol)
    z0, x0 = ops.at_margin_update(zm, xm, gm, pz, pg, th)
    z1, x1 = hiplib.at_margin_update(zm, xm, gm, pz, pg, th)
    assert torch.equal(z0, z1) and torch.equal(x0, x1)


# --- 5. csr_grad_from_mult ----------------------------------------------------------

@pytest.fixture(scope="module")
def heavy_csr():
    """n=5000 CSR rows with column 0 present in every row: one column far
    above the heavy-column threshold (task split + in-order combine)."""
    shard, _ = generate_csr_problem(n=5000, d=3001, nnz_per_row=9, seed=23,
                                    device=DEV)
    col = shard.col.clone()
    col[::9] = 0  # first (smallest) index of every row -> still sorted
    return CSRShard(shard.rowptr, col, shard.val, shard.labels, 3001)


def test_csr_grad_from_mult(heavy_csr):
    from sparkagd_amd.ops import hiplib

    sh = heavy_csr
    assert sh.csc_heavy["task_idx"].numel() >= 5000 // sh.CSC_TASK_S
    g = _gen(5)
    w = torch.randn(sh.d, generator=g, device=DEV, dtype=torch.float32) * 0.3
    z = sh.margins(w)
    mult, _ = ops.multiplier_loss_sum(z, sh.labels, ops.LOSS_LOGISTIC)
    args = (sh.rowptr, sh.col, sh.val, z, sh.labels, ops.LOSS_LOGISTIC, None, sh.d)
    want_csc, _ = hiplib.csr_eval_from_margins(*args, csc=sh.csc,
                                               csc_heavy=sh.csc_heavy)
    got_csc = ops.csr_grad_from_mult(sh.rowptr, sh.col, sh.val, mult, sh.d,
                                     csc=sh.csc, csc_heavy=sh.csc_heavy)
    assert torch.equal(got_csc, want_csc)
    assert torch.equal(sh.grad_from_mult(mult), want_csc)
    # CSC copy without the task split: thread-per-column gather
    want_plain, _ = hiplib.csr_eval_from_margins(*args, csc=sh.csc)
    got_plain = ops.csr_grad_from_mult(sh.rowptr, sh.col, sh.val, mult, sh.d,
                                       csc=sh.csc)
    assert torch.equal(got_plain, want_plain)
    # atomic scatter
    want_at, _ = hiplib.csr_eval_from_margins(*args, csc=None)
    got_at = ops.csr_grad_from_mult(sh.rowptr, sh.col, sh.val, mult, sh.d)
    torch.testing.assert_close(got_at, want_at, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(got_at, want_csc, rtol=1e-4, atol=1e-4)


# --- 6. InterceptShard.eval ------------------------------------------------------------

N6, D6 = 4096, 64


@pytest.fixture(scope="module")
def oracle6():
    """Shared CPU problem: f32 features (40% zeros so the CSR parts are
    sparse), unbalanced labels, weights, mask, [w; b]."""
    g = torch.Generator().manual_seed(61)
    A = torch.randn(N6, D6, generator=g) * (torch.rand(N6, D6, generator=g) >= 0.4)
    y = (torch.rand(N6, generator=g) < 0.8).to(torch.float32)
    sw = torch.rand(N6, generator=g) * 2.0
    mask = (torch.rand(N6, generator=g) < 0.5).to(torch.uint8)
    wb = torch.randn(D6 + 1, generator=g, dtype=F64) / math.sqrt(D6)
    return A, y, sw, mask, wb


def _oracle_eval(A_used, y, wb, loss_type, mask=None, sw=None):
    """CPU f64 eval on the ones-appended copy of the features as stored."""
    X = torch.cat([A_used.to(F64), torch.ones(A_used.shape[0], 1, dtype=F64)], dim=1)
    return DenseShard(X, y.to(F64), sw).eval(wb, loss_type, mask)


def _csr_gpu(A, y, sw=None):
    s = A.to_sparse_csr()
    return CSRShard(s.crow_indices().to(DEV), s.col_indices().to(DEV),
                    s.values().to(DEV), y.to(DEV), A.shape[1],
                    sample_weight=None if sw is None else sw.to(DEV))


# (grad rtol, grad atol, loss/count rtol, loss/count atol) of the matching
# eval tests in test_gpu_kernels.py
TOL6 = {
    "bf16": (2e-4, 2e-3, 1e-5, 1e-6),   # test_dense_eval_matches_reference
    "f32": (2e-4, 2e-3, 1e-5, 1e-6),
    "f64": (1e-9, 1e-9, 1e-9, 1e-9),    # test_dense_eval_f64
    "fp8": (2e-4, 2e-3, 1e-5, 1e-5),    # test_dense_eval_fp8
    "csr": (1e-4, 1e-3, 1e-5, 1e-6),    # test_csr_eval_matches_reference
    "mixed": (2e-4, 2e-3, 1e-5, 1e-6),  # bf16 dense part + CSR part
}


@pytest.mark.parametrize("kind", list(TOL6))
def test_intercept_shard_eval(kind, oracle6):
    A, y, sw, mask, wb = oracle6
    wdt = F64 if kind == "f64" else torch.float32
    if kind in ("bf16", "fp8"):
        dt = torch.bfloat16 if kind == "bf16" else torch.float8_e4m3fn
        stored = A.to(dt)
        inner = DenseShard(stored.to(DEV), y.to(DEV), sw.to(DEV))
        used = stored.to(torch.float32)
    elif kind in ("f32", "f64"):
        inner = DenseShard(A.to(DEV, wdt), y.to(DEV), sw.to(DEV))
        used = A
    elif kind == "csr":
        inner = _csr_gpu(A, y, sw)
        used = A
    else:
        k = 1501  # odd split: the CSR part's mult slice is not 16-byte aligned
        top = A[:k].to(torch.bfloat16)
        inner = MixedShard([DenseShard(top.to(DEV), y[:k].to(DEV), sw[:k].to(DEV)),
                            _csr_gpu(A[k:], y[k:], sw[k:])])
        used = torch.cat([top.to(torch.float32), A[k:]])
    sh = InterceptShard(inner)
    assert sh.d == D6 + 1 and sh.n == N6
    w_gpu = wb.to(DEV, wdt)
    gr, ga, lr, la = TOL6[kind]
    for loss_type, m in ((ops.LOSS_LOGISTIC, None),
                         (ops.LOSS_LEAST_SQUARES, mask)):
        g_o, lc_o = _oracle_eval(used, y, w_gpu.double().cpu(), loss_type, m, sw)
        g_h, lc_h = sh.eval(w_gpu, loss_type, None if m is None else m.to(DEV))
        assert g_h.shape == (D6 + 1,) and g_h.dtype == wdt
        g_h = g_h.double().cpu()
        print(kind, loss_type, "Σmult", float(g_h[-1]), float(g_o[-1]),
              "max|dgrad|", float((g_h - g_o).abs().max()))
        torch.testing.assert_close(g_h[:-1], g_o[:-1], rtol=gr, atol=ga)
        torch.testing.assert_close(lc_h.cpu(), lc_o, rtol=lr, atol=la)
        assert abs(float(g_h[-1] - g_o[-1])) <= 1e-5 * abs(float(g_o[-1]))
        # loss-only evaluation agrees and skips the gradient
        none, lc2 = sh.eval(w_gpu, loss_type, None if m is None else m.to(DEV),
                            need_grad=False)
        assert none is None and torch.equal(lc2, lc_h)


# --- 7. end-to-end training ---------------------------------------------------------------

def test_train_with_intercept_gpu_matches_cpu_oracle():
    g = torch.Generator().manual_seed(71)
    n, d = 10000, 64
    A = torch.randn(n, d, generator=g, dtype=F64)
    w_true = torch.randn(d, generator=g, dtype=F64) / math.sqrt(d)
    y = (torch.rand(n, generator=g, dtype=F64)
         < torch.sigmoid(A @ w_true + 1.5)).to(F64)
    kw = dict(intercept=True, reg_param=0.05, num_iterations=10,
              convergence_tol=1e-12)
    mc = LogisticRegressionWithAGD.train(DenseShard(A, y), **kw)
    mg = LogisticRegressionWithAGD.train(
        DenseShard(A.to(DEV, torch.float32), y.to(DEV)), **kw)
    assert len(mc.loss_history) == len(mg.loss_history) == 10
    assert mg.weights.shape == (d,) and mg.weights.is_cuda
    assert_rel(mc.loss_history[-1], mg.loss_history[-1], 1e-3,
               "GPU f32 vs CPU f64 final loss")
    wg = torch.cat([mg.weights.double().cpu(), torch.tensor([mg.intercept], dtype=F64)])
    wc = torch.cat([mc.weights, torch.tensor([mc.intercept], dtype=F64)])
    torch.testing.assert_close(wg, wc, rtol=5e-3, atol=5e-3)
    assert mc.intercept > 0.5


def test_intercept_margin_tracking_matches_untracked_gpu():
    shard, _ = generate_dense_problem(n=40000, d=512, seed=5, device=DEV,
                                      dtype=torch.bfloat16)
    sh = InterceptShard(shard)
    w0 = torch.zeros(sh.d, device=DEV, dtype=torch.float32)
    w0[-1] = 0.5  # a bias the (1 - pz)*z_b correction has to carry
    args = (sh, LogisticGradient(), FreeTailUpdater(SquaredL2Updater()), 1e-12,
            8, 0.05, w0, 1.0, math.inf, 0.5, 0.9, True)
    w_t, h_t = run(*args)
    w_u, h_u = run(*args, track_margins=False)
    assert len(h_t) == len(h_u)
    for a, b in zip(h_t, h_u):
        assert abs(a - b) < 2e-4 * max(1.0, abs(b)), (a, b)
    torch.testing.assert_close(w_t, w_u, rtol=5e-3, atol=5e-3)


# --- 8. no new host traffic -------------------------------------------------------------------

def _memcpy_counts(fn):
    from torch.profiler import ProfilerActivity, profile

    fn()  # warmup (allocator, kernel caches)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    h2d = d2h = 0
    for e in prof.key_averages():
        key = e.key.lower().replace(" ", "")
        if "memcpy" not in key:
            continue
        if "htod" in key:
            h2d += e.count
        elif "dtoh" in key:
            d2h += e.count
    return h2d, d2h


def test_intercept_adds_no_host_traffic():
    """beta=1 and convergence_tol=0 fix the evaluation count (no
    backtracking, no early stop), so the two runs make the same number of
    scalar fetches; the intercept adds none and copies nothing to the device."""
    d = 100_000
    shard, _ = generate_dense_problem(n=512, d=d, seed=13, device=DEV,
                                      dtype=torch.bfloat16)

    def plain():
        w0 = torch.zeros(d, device=DEV, dtype=torch.float32)
        run(shard, LogisticGradient(), SquaredL2Updater(), 0.0, 4, 1e-3, w0,
            1.0, math.inf, 1.0, 0.9, True)

    def with_intercept():
        w0 = torch.zeros(d + 1, device=DEV, dtype=torch.float32)
        run(InterceptShard(shard), LogisticGradient(),
            FreeTailUpdater(SquaredL2Updater()), 0.0, 4, 1e-3, w0,
            1.0, math.inf, 1.0, 0.9, True)

    h2d_p, d2h_p = _memcpy_counts(plain)
    h2d_i, d2h_i = _memcpy_counts(with_intercept)
    print("plain (h2d, d2h)", (h2d_p, d2h_p), "intercept", (h2d_i, d2h_i))
    assert d2h_p > 0, "the profiler must see the scalar fetches"
    assert h2d_i == 0, f"{h2d_i} host->device copies in an intercept run"
    assert h2d_p == 0
    assert d2h_i == d2h_p, (d2h_i, d2h_p)
