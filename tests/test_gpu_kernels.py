"""HIP kernel numerics: every kernel vs the plain-PyTorch fp32/fp64 oracle
(`ops.reference`) on the same data."""

import math

import pytest
import torch

from sparkagd_amd import ops
from sparkagd_amd.data import generate_csr_problem

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _mk_dense(n, d, dtype, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    A = torch.randn((n, d), generator=g, device=DEV, dtype=torch.float32)
    y = (torch.randn(n, generator=g, device=DEV) > 0).to(torch.float32)
    w = torch.randn(d, generator=g, device=DEV, dtype=torch.float32) / math.sqrt(d)
    return A.to(dtype).contiguous(), y, w


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("loss_type", [ops.LOSS_LOGISTIC, ops.LOSS_LEAST_SQUARES, ops.LOSS_HINGE, ops.LOSS_SMOOTH_HINGE])
def test_dense_eval_matches_reference(dtype, loss_type):
    from sparkagd_amd.ops import hiplib, reference

    A, y, w = _mk_dense(4096, 512, dtype)
    grad_h, lc_h = hiplib.dense_eval(A, y, w, loss_type)
    grad_r, lc_r = reference.dense_eval(A, y, w, loss_type)
    torch.testing.assert_close(grad_h, grad_r, rtol=2e-4, atol=2e-3)
    torch.testing.assert_close(lc_h, lc_r, rtol=1e-5, atol=1e-6)
    assert float(lc_h[1]) == 4096


@pytest.mark.parametrize("n,d", [(4096, 13), (33, 7)])
def test_dense_eval_unaligned_d(n, d):
    """d not a multiple of the 16-B lane width -> scalar (W=1) kernel path."""
    from sparkagd_amd.ops import hiplib, reference

    A, y, w = _mk_dense(n, d, torch.float32)
    grad_h, lc_h = hiplib.dense_eval(A, y, w, ops.LOSS_LOGISTIC)
    grad_r, lc_r = reference.dense_eval(A, y, w, ops.LOSS_LOGISTIC)
    torch.testing.assert_close(grad_h, grad_r, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(lc_h, lc_r, rtol=1e-6, atol=1e-8)


def test_dense_eval_thin_n_fat_d_column_slabs():
    """n << CU count forces the column-slab margins path (atomic accumulate)."""
    from sparkagd_amd.ops import hiplib, reference

    A, y, w = _mk_dense(96, 100352, torch.float32, seed=3)
    grad_h, lc_h = hiplib.dense_eval(A, y, w, ops.LOSS_LOGISTIC)
    grad_r, lc_r = reference.dense_eval(A, y, w, ops.LOSS_LOGISTIC)
    torch.testing.assert_close(grad_h, grad_r, rtol=3e-4, atol=3e-4)
    torch.testing.assert_close(lc_h, lc_r, rtol=1e-5, atol=1e-6)


def test_dense_eval_f64():
    from sparkagd_amd.ops import hiplib, reference

    g = torch.Generator(device=DEV).manual_seed(1)
    A = torch.randn((2048, 130), generator=g, device=DEV, dtype=torch.float64)
    y = (torch.randn(2048, generator=g, device=DEV) > 0).to(torch.float32)
    w = torch.randn(130, generator=g, device=DEV, dtype=torch.float64)
    grad_h, lc_h = hiplib.dense_eval(A, y, w, ops.LOSS_LOGISTIC)
    grad_r, lc_r = reference.dense_eval(A, y.to(torch.float64), w, ops.LOSS_LOGISTIC)
    # fp64 path: differences only from fma contraction / summation order /
    # device-vs-host libm ulps
    torch.testing.assert_close(grad_h, grad_r, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(lc_h, lc_r, rtol=1e-9, atol=1e-9)


def test_dense_eval_sample_weight():
    from sparkagd_amd.ops import hiplib, reference

    A, y, w = _mk_dense(5000, 64, torch.float32, seed=6)
    g = torch.Generator(device=DEV).manual_seed(10)
    sw = torch.rand(5000, generator=g, device=DEV) * 2.0
    grad_h, lc_h = hiplib.dense_eval(A, y, w, ops.LOSS_LOGISTIC, sample_weight=sw)
    grad_r, lc_r = reference.dense_eval(A, y, w, ops.LOSS_LOGISTIC, sample_weight=sw)
    torch.testing.assert_close(grad_h, grad_r, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(lc_h, lc_r, rtol=1e-6, atol=1e-6)


def test_dense_eval_masked():
    from sparkagd_amd.ops import hiplib, reference

    A, y, w = _mk_dense(5000, 64, torch.float32, seed=5)
    g = torch.Generator(device=DEV).manual_seed(9)
    mask = (torch.rand(5000, generator=g, device=DEV) < 0.4).to(torch.uint8)
    grad_h, lc_h = hiplib.dense_eval(A, y, w, ops.LOSS_LEAST_SQUARES, mask)
    grad_r, lc_r = reference.dense_eval(A, y, w, ops.LOSS_LEAST_SQUARES, mask)
    torch.testing.assert_close(grad_h, grad_r, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(lc_h, lc_r, rtol=1e-6, atol=1e-8)
    assert float(lc_h[1]) == float(mask.sum())


def test_dense_grad_deterministic():
    """The dense A^T·m partial-slab path is bitwise reproducible."""
    from sparkagd_amd.ops import hiplib

    A, y, w = _mk_dense(8192, 256, torch.bfloat16, seed=7)
    g1, lc1 = hiplib.dense_eval(A, y, w, ops.LOSS_LOGISTIC)
    g2, lc2 = hiplib.dense_eval(A, y, w, ops.LOSS_LOGISTIC)
    assert torch.equal(g1, g2)
    assert torch.equal(lc1, lc2)


@pytest.mark.parametrize("loss_type", [ops.LOSS_LOGISTIC, ops.LOSS_HINGE])
def test_csr_eval_matches_reference(loss_type):
    from sparkagd_amd.ops import hiplib, reference

    shard, _ = generate_csr_problem(n=20000, d=50000, nnz_per_row=32, seed=11, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(2)
    w = torch.randn(50000, generator=g, device=DEV, dtype=torch.float32) * 0.1
    grad_h, lc_h = hiplib.csr_eval(shard.rowptr, shard.col, shard.val, shard.labels, w, loss_type)
    grad_r, lc_r = reference.csr_eval(shard.rowptr, shard.col, shard.val, shard.labels, w, loss_type, d=50000)
    torch.testing.assert_close(grad_h, grad_r, rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(lc_h, lc_r, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("n,d", [(8192, 1024), (100, 20000)])
def test_margins_mfma_matches_valu(n, d, monkeypatch):
    """The MFMA margins kernel (32x32x16 bf16, LDS-staged w tiles) agrees with
    the VALU kernel up to w's bf16 rounding (the MFMA input format)."""
    from sparkagd_amd.ops import hiplib, reference

    A, y, w = _mk_dense(n, d, torch.bfloat16, seed=31)
    monkeypatch.setenv("SPARKAGD_MARGINS_ALGO", "1")
    g1, lc1 = hiplib.dense_eval(A, y, w, ops.LOSS_LOGISTIC)
    monkeypatch.setenv("SPARKAGD_MARGINS_ALGO", "2")
    g2, lc2 = hiplib.dense_eval(A, y, w, ops.LOSS_LOGISTIC)
    monkeypatch.delenv("SPARKAGD_MARGINS_ALGO")
    # oracle with w pre-rounded to bf16 (what the matrix core consumes)
    w_rounded = w.to(torch.bfloat16).to(torch.float32)
    gr, lcr = reference.dense_eval(A, y, w_rounded, ops.LOSS_LOGISTIC)
    torch.testing.assert_close(g2, gr, rtol=3e-4, atol=3e-3)
    torch.testing.assert_close(lc2, lcr, rtol=1e-5, atol=1e-5)
    # NOTE: g2 vs g1 (VALU, fp32 w) differ by the full w-rounding
    # perturbation, which grows with n — the oracle comparison above is the
    # correctness check; here only the count must agree.
    assert g1 is not None
    assert float(lc1[1]) == float(lc2[1]) == n


@pytest.mark.parametrize("loss_type", [ops.LOSS_LOGISTIC, ops.LOSS_LEAST_SQUARES])
def test_dense_eval_fp8(loss_type):
    """fp8 e4m3fn shard path (hardware v_cvt_pk_f32_fp8 decodes) vs the
    oracle evaluated on the same quantized values."""
    from sparkagd_amd.ops import hiplib, reference

    A32, y, w = _mk_dense(4096, 512, torch.float32, seed=41)
    A8 = A32.to(torch.float8_e4m3fn).contiguous()
    grad_h, lc_h = hiplib.dense_eval(A8, y, w, loss_type)
    grad_r, lc_r = reference.dense_eval(A8, y, w, loss_type)
    torch.testing.assert_close(grad_h, grad_r, rtol=2e-4, atol=2e-3)
    torch.testing.assert_close(lc_h, lc_r, rtol=1e-5, atol=1e-5)
    # loss-only and unaligned-d scalar decode path
    _, lc2 = hiplib.dense_eval(A8, y, w, loss_type, need_grad=False)
    assert torch.equal(lc_h, lc2)
    A8u = A8[:, :500].contiguous()
    g_u, lc_u = hiplib.dense_eval(A8u, y, w[:500].contiguous(), loss_type)
    g_ur, lc_ur = reference.dense_eval(A8u, y, w[:500], loss_type)
    torch.testing.assert_close(g_u, g_ur, rtol=2e-4, atol=2e-3)


def test_dense_eval_loss_only():
    """need_grad=False returns the identical loss/count without the A^T·m pass."""
    from sparkagd_amd.ops import hiplib

    A, y, w = _mk_dense(4096, 512, torch.bfloat16, seed=21)
    gfull, lc_full = hiplib.dense_eval(A, y, w, ops.LOSS_LOGISTIC, need_grad=True)
    gnone, lc_loss = hiplib.dense_eval(A, y, w, ops.LOSS_LOGISTIC, need_grad=False)
    assert gnone is None and gfull is not None
    assert torch.equal(lc_full, lc_loss)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("k", [3, 8])
def test_multiclass_kernels_match_oracle(dtype, k, monkeypatch):
    """margins_multi + multiplier_multi + grad_multi vs the torch oracle
    (includes non-multiple-of-4 K -> class padding). For bf16 shards the
    default margins path is the hipBLASLt GEMM with bf16-rounded W, so the
    oracle uses the same rounded W; the f32-weights VALU kernel is checked
    separately under SPARKAGD_MULTI_MARGINS=valu."""
    from sparkagd_amd.ops import multiclass as mc
    from sparkagd_amd.ops import hiplib

    g = torch.Generator(device=DEV).manual_seed(51)
    n, d = 4096, 512
    A = torch.randn((n, d), generator=g, device=DEV).to(dtype).contiguous()
    y = torch.randint(0, k, (n,), generator=g, device=DEV).to(torch.float32)
    W = (torch.randn(d * k, generator=g, device=DEV) / math.sqrt(d)).contiguous()
    # oracle weights matching the compute path: the GEMM route rounds W to bf16
    Wr = W.reshape(d, k).to(torch.bfloat16).to(torch.float32).reshape(-1) \
        if dtype == torch.bfloat16 else W

    def check_grad(gh, gr):
        if dtype == torch.bfloat16:
            # GEMM grad rounds the multipliers to bf16 -> norm-relative bound
            assert float(torch.norm(gh - gr)) < 3e-3 * float(torch.norm(gr))
        else:
            torch.testing.assert_close(gh, gr, rtol=3e-4, atol=3e-3)

    grad_h, lc_h = mc.eval_multi(A, y, W, k)
    grad_r, lc_r = mc.ref_eval_multi(A, y, Wr, k)
    check_grad(grad_h, grad_r)
    torch.testing.assert_close(lc_h, lc_r, rtol=1e-5, atol=1e-5)
    # loss-only agrees
    _, lc2 = mc.eval_multi(A, y, W, k, need_grad=False)
    torch.testing.assert_close(lc_h, lc2)
    # with mask + sample weights
    mask = (torch.rand(n, generator=g, device=DEV) < 0.5).to(torch.uint8)
    sw = torch.rand(n, generator=g, device=DEV) * 2
    gh, lh = mc.eval_multi(A, y, W, k, mask=mask, sample_weight=sw)
    gr, lr = mc.ref_eval_multi(A, y, Wr, k, mask=mask, sample_weight=sw)
    check_grad(gh, gr)
    torch.testing.assert_close(lh, lr, rtol=1e-5, atol=1e-5)
    # the exact-f32 VALU kernels are still selectable and tight
    monkeypatch.setenv("SPARKAGD_MULTI_MARGINS", "valu")
    monkeypatch.setenv("SPARKAGD_MULTI_GRAD", "valu")
    gv, lv = mc.eval_multi(A, y, W, k)
    grad_f32 = mc.ref_eval_multi(A, y, W, k)
    torch.testing.assert_close(gv, grad_f32[0], rtol=3e-4, atol=3e-3)
    torch.testing.assert_close(lv, grad_f32[1], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("k", [10, 16])
def test_multiclass_gemm_margins_match_valu(k, monkeypatch):
    """The GEMM margins path equals the VALU kernel run on bf16-rounded
    weights (same math, different engine), and is run-to-run deterministic."""
    from sparkagd_amd.ops import multiclass as mc

    g = torch.Generator(device=DEV).manual_seed(52)
    n, d = 8192, 768
    A = torch.randn((n, d), generator=g, device=DEV).to(torch.bfloat16).contiguous()
    W = (torch.randn(d * k, generator=g, device=DEV) / math.sqrt(d)).contiguous()
    Wr = W.reshape(d, k).to(torch.bfloat16).to(torch.float32).reshape(-1)

    monkeypatch.setenv("SPARKAGD_MULTI_MARGINS", "gemm")
    zg = mc.margins_multi(A, W, k)
    zg2 = mc.margins_multi(A, W, k)
    assert torch.equal(zg, zg2), "hipBLASLt margins GEMM must be deterministic"
    monkeypatch.setenv("SPARKAGD_MULTI_MARGINS", "valu")
    zv = mc.margins_multi(A, Wr, k)
    torch.testing.assert_close(zg, zv, rtol=1e-4, atol=1e-4)

    # TN grad GEMM: deterministic, and equals the VALU kernel fed the same
    # bf16-rounded multipliers
    from sparkagd_amd.ops import hiplib

    y = torch.randint(0, k, (n,), generator=g, device=DEV).to(torch.float32)
    monkeypatch.setenv("SPARKAGD_MULTI_GRAD", "gemm")
    g1, lc1 = mc.eval_multi_from_margins(A, zg, y, k)
    g2, lc2 = mc.eval_multi_from_margins(A, zg, y, k)
    assert torch.equal(g1, g2), "hipBLASLt TN grad GEMM must be deterministic"
    torch.testing.assert_close(lc1, lc2)
    monkeypatch.setenv("SPARKAGD_MULTI_GRAD", "valu")
    kc = mc.padded_k(k)
    M = torch.empty(n * kc, dtype=torch.float32, device=DEV)
    lib = hiplib.load()
    lc = torch.zeros(2, dtype=torch.float64, device=DEV)
    rc = lib.agd_multiplier_multi(
        hiplib._ptr(zg.contiguous()), hiplib._ptr(y.contiguous()), None, None,
        n, k, kc, hiplib._ptr(M), hiplib._ptr(lc),
        hiplib._ptr(hiplib._red_ws(DEV)), hiplib._stream(A))
    assert rc == 0
    Mr = M.to(torch.bfloat16).to(torch.float32)  # what the GEMM path consumed
    gradp = torch.empty(A.shape[1] * kc, dtype=torch.float32, device=DEV)
    n_rb = int(lib.agd_multi_rowblocks(n, A.shape[1], kc))
    part = torch.empty(n_rb * A.shape[1] * kc, dtype=torch.float32, device=DEV) if n_rb > 1 else gradp
    rc = lib.agd_grad_multi(hiplib._ptr(A), 0, hiplib._ptr(Mr), n, A.shape[1],
                            kc, hiplib._ptr(part), n_rb, hiplib._ptr(gradp),
                            hiplib._stream(A))
    assert rc == 0
    gv = gradp.reshape(A.shape[1], kc)[:, :k].reshape(-1).contiguous()
    torch.testing.assert_close(g1, gv, rtol=3e-4, atol=3e-3)


@pytest.mark.parametrize("k", [3, 16])
def test_csr_multiclass_kernels_match_oracle(k):
    """k_csr_margins_multi + k_csc_grad_multi vs the CPU-style oracle, plus
    bitwise run-to-run determinism of the CSC-gather gradient."""
    from sparkagd_amd.data import generate_multiclass_csr_problem
    from sparkagd_amd.ops import multiclass as mc
    from sparkagd_amd import MultinomialLogisticGradient

    shard, _ = generate_multiclass_csr_problem(20000, 30000, 24,
                                               num_classes=k, seed=31,
                                               device=DEV)
    g = torch.Generator(device=DEV).manual_seed(32)
    W = (torch.randn(shard.d * k, generator=g, device=DEV) /
         math.sqrt(24)).contiguous()
    grad = MultinomialLogisticGradient(k)
    gh, lh = grad.eval(shard, W)
    # oracle on the same GPU tensors (plain torch index_add path)
    zf = mc.ref_csr_margins_multi(shard.rowptr, shard.col, shard.val, W, k,
                                  shard.d).reshape(-1, k)
    m, lr = mc.ref_multiplier_multi(zf, shard.labels)
    gr = mc.ref_csr_grad_multi(shard.rowptr, shard.col, shard.val, m, shard.d)
    torch.testing.assert_close(gh, gr, rtol=3e-4, atol=3e-4)
    torch.testing.assert_close(lh, lr, rtol=1e-6, atol=1e-6)
    # determinism: identical bits across repeated evaluations
    gh2, lh2 = grad.eval(shard, W)
    assert torch.equal(gh, gh2) and torch.equal(lh, lh2)
    # loss-only
    gn, ln = grad.eval(shard, W, need_grad=False)
    assert gn is None
    torch.testing.assert_close(lh, ln)


def test_csr_multiclass_bf16_w_gather(monkeypatch):
    """The optional bf16 W-row gather path matches the oracle with
    bf16-rounded weights (measured perf-neutral — BACKLOG.md — but kept
    selectable)."""
    from sparkagd_amd.data import generate_multiclass_csr_problem
    from sparkagd_amd.ops import multiclass as mc

    k = 8
    shard, _ = generate_multiclass_csr_problem(10000, 20000, 16,
                                               num_classes=k, seed=37,
                                               device=DEV)
    g = torch.Generator(device=DEV).manual_seed(38)
    W = (torch.randn(shard.d * k, generator=g, device=DEV) /
         math.sqrt(16)).contiguous()
    Wr = W.reshape(shard.d, k).to(torch.bfloat16).to(torch.float32).reshape(-1)
    monkeypatch.setenv("SPARKAGD_CSR_MULTI_W", "bf16")
    zb = mc.csr_margins_multi(shard, W, k)
    monkeypatch.setenv("SPARKAGD_CSR_MULTI_W", "f32")
    zr = mc.csr_margins_multi(shard, Wr, k)
    torch.testing.assert_close(zb, zr, rtol=1e-6, atol=1e-6)


def test_csr_multiclass_large_k():
    """K > 32 CSR runs the gather kernels per 32-class chunk."""
    from sparkagd_amd.data import generate_multiclass_csr_problem
    from sparkagd_amd.ops import multiclass as mc
    from sparkagd_amd import MultinomialLogisticGradient

    k = 40
    shard, _ = generate_multiclass_csr_problem(8000, 10000, 16,
                                               num_classes=k, seed=35,
                                               device=DEV)
    g = torch.Generator(device=DEV).manual_seed(36)
    W = (torch.randn(shard.d * k, generator=g, device=DEV) /
         math.sqrt(16)).contiguous()
    grad = MultinomialLogisticGradient(k)
    gh, lh = grad.eval(shard, W)
    zf = mc.ref_csr_margins_multi(shard.rowptr, shard.col, shard.val, W, k,
                                  shard.d).reshape(-1, k)
    m, lr = mc.ref_multiplier_multi(zf, shard.labels)
    gr = mc.ref_csr_grad_multi(shard.rowptr, shard.col, shard.val, m, shard.d)
    torch.testing.assert_close(gh, gr, rtol=3e-4, atol=3e-4)
    torch.testing.assert_close(lh, lr, rtol=1e-6, atol=1e-6)
    gh2, lh2 = grad.eval(shard, W)
    assert torch.equal(gh, gh2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_multiclass_large_k(dtype):
    """K > 32 runs GEMM-shaped on the GPU (hipBLASLt / rocBLAS margins+grad,
    torch multiplier stage) — vs the oracle."""
    from sparkagd_amd.ops import multiclass as mc

    g = torch.Generator(device=DEV).manual_seed(53)
    n, d, k = 8192, 768, 40
    A = torch.randn((n, d), generator=g, device=DEV).to(dtype).contiguous()
    y = torch.randint(0, k, (n,), generator=g, device=DEV).to(torch.float32)
    W = (torch.randn(d * k, generator=g, device=DEV) / math.sqrt(d)).contiguous()
    Wr = W.reshape(d, k).to(torch.bfloat16).to(torch.float32).reshape(-1) \
        if dtype == torch.bfloat16 else W

    gh, lh = mc.eval_multi(A, y, W, k)
    gr, lr = mc.ref_eval_multi(A, y, Wr, k)
    assert gh.numel() == d * k
    if dtype == torch.bfloat16:
        assert float(torch.norm(gh - gr)) < 3e-3 * float(torch.norm(gr))
    else:
        torch.testing.assert_close(gh, gr, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(lh, lr, rtol=1e-5, atol=1e-5)
    # mask + sample weights flow through the torch multiplier stage
    mask = (torch.rand(n, generator=g, device=DEV) < 0.5).to(torch.uint8)
    sw = torch.rand(n, generator=g, device=DEV) * 2
    gh2, lh2 = mc.eval_multi(A, y, W, k, mask=mask, sample_weight=sw)
    gr2, lr2 = mc.ref_eval_multi(A, y, Wr, k, mask=mask, sample_weight=sw)
    if dtype == torch.bfloat16:
        assert float(torch.norm(gh2 - gr2)) < 3e-3 * float(torch.norm(gr2))
    else:
        torch.testing.assert_close(gh2, gr2, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(lh2, lr2, rtol=1e-5, atol=1e-5)
    # loss-only
    gn, ln = mc.eval_multi(A, y, W, k, need_grad=False)
    assert gn is None
    torch.testing.assert_close(lh, ln)


def test_csr_csc_deterministic_vs_atomic():
    """The CSC-gather A^T·m equals the atomic-scatter path (tolerance) and is
    bitwise reproducible run-to-run (SURVEY.md §5 race-detection cross-check)."""
    from sparkagd_amd.ops import hiplib

    shard, _ = generate_csr_problem(n=30000, d=40000, nnz_per_row=24, seed=17, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    w = torch.randn(40000, generator=g, device=DEV, dtype=torch.float32) * 0.1
    args = (shard.rowptr, shard.col, shard.val, shard.labels, w, ops.LOSS_LOGISTIC, None, 40000)
    g_atomic, lc_a = hiplib.csr_eval(*args, csc=None)
    g_csc1, lc_c = hiplib.csr_eval(*args, csc=shard.csc)
    g_csc2, _ = hiplib.csr_eval(*args, csc=shard.csc)
    assert torch.equal(g_csc1, g_csc2)  # deterministic
    torch.testing.assert_close(g_csc1, g_atomic, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(lc_a, lc_c, rtol=0, atol=0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_axpby(dtype):
    from sparkagd_amd.ops import hiplib

    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(100003, generator=g, device=DEV, dtype=dtype)
    y = torch.randn(100003, generator=g, device=DEV, dtype=dtype)
    out = hiplib.axpby(0.3, x, -1.7, y)
    torch.testing.assert_close(out, 0.3 * x - 1.7 * y)


@pytest.mark.parametrize("kind", [ops.PROX_SIMPLE, ops.PROX_L1, ops.PROX_SQUARED_L2, ops.PROX_ELASTIC_NET])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_prox(kind, dtype):
    from sparkagd_amd.ops import hiplib, reference

    g = torch.Generator(device=DEV).manual_seed(4)
    w = torch.randn(70001, generator=g, device=DEV, dtype=dtype)
    gr = torch.randn(70001, generator=g, device=DEV, dtype=dtype)
    lam2 = 0.11 if kind == ops.PROX_ELASTIC_NET else 0.0
    out_h, reg_h = hiplib.prox(kind, w, gr, 0.37, 0.21, lam2)
    out_r, reg_r = reference.prox(kind, w, gr, 0.37, 0.21, lam2)
    torch.testing.assert_close(out_h, out_r, rtol=1e-6, atol=1e-6)
    # reg tolerance: at f32 the elementwise w' differs from torch by fma
    # contraction (1 ulp); the f64 reg sum of 70k such terms walks ~1e-5 abs
    torch.testing.assert_close(reg_h, reg_r, rtol=5e-6, atol=5e-6)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_fused_scalars_and_dot_diff(dtype):
    from sparkagd_amd.ops import hiplib, reference

    g = torch.Generator(device=DEV).manual_seed(6)
    vecs = [torch.randn(123457, generator=g, device=DEV, dtype=dtype) for _ in range(4)]
    out_h = hiplib.fused_scalars(*vecs)
    out_r = reference.fused_scalars(*vecs)
    torch.testing.assert_close(out_h, out_r, rtol=1e-10, atol=1e-8)

    gx = torch.randn(123457, generator=g, device=DEV, dtype=dtype)
    dd_h = hiplib.dot_diff(vecs[0], vecs[1], gx, vecs[2])
    dd_r = reference.dot_diff(vecs[0], vecs[1], gx, vecs[2])
    torch.testing.assert_close(dd_h, dd_r, rtol=1e-10, atol=1e-8)


def test_gpu_dispatch_uses_hip():
    """ops dispatch on CUDA tensors must go through the HIP library (and the
    library must actually be loadable on a GPU box)."""
    assert ops.hip_available()
    A, y, w = _mk_dense(256, 64, torch.float32)
    grad, lc = ops.dense_eval(A, y, w, ops.LOSS_LOGISTIC)
    assert grad.is_cuda and float(lc[1]) == 256


@pytest.mark.parametrize("k", [50, 100, 333])
def test_multiplier_multi_anyk_matches_oracle(k):
    """The generic-K (wave-per-row) multiplier kernel vs the torch oracle:
    padded M (exact-zero pad columns), loss_count, mask and sample-weight
    composition, run-to-run determinism. K > 32 previously ran a ~6-kernel
    torch stage."""
    from sparkagd_amd.ops import hiplib
    from sparkagd_amd.ops import multiclass as mc

    g = torch.Generator(device=DEV).manual_seed(91)
    n = 20000
    kc = mc.padded_k(k)
    assert kc > 32
    z = torch.randn(n * kc, generator=g, device=DEV) * 3.0
    z = z.reshape(n, kc)
    z[:, k:] = 0.0  # pad columns (opaque, but keep them finite)
    y = torch.randint(0, k, (n,), generator=g, device=DEV).to(torch.float32)
    mask = (torch.rand(n, generator=g, device=DEV) < 0.7).to(torch.uint8)
    sw = torch.rand(n, generator=g, device=DEV) + 0.5

    for m_arg, w_arg in [(None, None), (mask, None), (None, sw), (mask, sw)]:
        M, lc = hiplib.multiplier_multi(z.reshape(-1), y, k, kc, m_arg, w_arg)
        m_ref, lc_ref = mc.ref_multiplier_multi(z[:, :k], y, m_arg, w_arg)
        M2 = M.reshape(n, kc)
        assert torch.all(M2[:, k:] == 0.0), "pad columns must be exact zeros"
        torch.testing.assert_close(M2[:, :k], m_ref, rtol=2e-5, atol=2e-6)
        torch.testing.assert_close(lc, lc_ref, rtol=1e-6, atol=1e-6)
        Mb, lcb = hiplib.multiplier_multi(z.reshape(-1), y, k, kc, m_arg, w_arg)
        assert torch.equal(M, Mb) and torch.equal(lc, lcb)


def test_csc_grad_skew_matches_oracle(monkeypatch):
    """Skew-robust CSC gradient (heavy-column split + in-order combine) vs
    the torch oracle on a deliberately skewed shard, with the thresholds
    lowered so the heavy path engages at test scale; bitwise determinism
    and equality-of-structure with the unsplit path."""
    from sparkagd_amd.data import CSRShard
    from sparkagd_amd.ops import reference as ref

    monkeypatch.setattr(CSRShard, "CSC_HEAVY_T", 128)
    monkeypatch.setattr(CSRShard, "CSC_TASK_S", 128)

    g = torch.Generator(device=DEV).manual_seed(17)
    n, d, nnz_per_row = 30000, 5000, 16
    nnz = n * nnz_per_row
    # ~40% of nnz land in 8 hot columns, rest uniform
    hot = torch.randint(0, 8, (nnz,), generator=g, device=DEV, dtype=torch.int32)
    uni = torch.randint(0, d, (nnz,), generator=g, device=DEV, dtype=torch.int32)
    pick = torch.rand(nnz, generator=g, device=DEV) < 0.4
    col = torch.where(pick, hot * 601 % d, uni).to(torch.int32)
    col = col.view(n, nnz_per_row).sort(dim=1).values.reshape(-1)
    val = torch.randn(nnz, generator=g, device=DEV)
    rowptr = torch.arange(0, nnz + 1, nnz_per_row, device=DEV, dtype=torch.int32)
    labels = (torch.rand(n, generator=g, device=DEV) < 0.5).float()
    shard = CSRShard(rowptr, col, val, labels, d)
    assert shard.csc_heavy is not None, "heavy path must engage on this shard"
    assert shard.csc_heavy["task_idx"].numel() > shard.csc_heavy["cols"].numel()

    w = torch.randn(d, generator=g, device=DEV) * 0.05
    gh, lh = shard.eval(w, 0)  # logistic
    gr, lr = ref.csr_eval(shard.rowptr, shard.col, shard.val, labels, w, 0,
                          None, d)
    torch.testing.assert_close(lh, lr.to(lh.dtype), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(gh, gr.to(gh.dtype), rtol=2e-4, atol=2e-4)
    gh2, lh2 = shard.eval(w, 0)
    assert torch.equal(gh, gh2) and torch.equal(lh, lh2)

    # unsplit (thresholds back to default => heavy structure absent at this
    # scale) must agree to fp-reassociation level
    monkeypatch.setattr(CSRShard, "CSC_HEAVY_T", 2048)
    monkeypatch.setattr(CSRShard, "CSC_TASK_S", 2048)
    shard2 = CSRShard(rowptr, col, val, labels, d)
    assert shard2.csc_heavy["task_idx"].numel() > 0  # hottest col >> 2048
    monkeypatch.setattr(CSRShard, "CSC_HEAVY_T", 10**9)
    shard3 = CSRShard(rowptr, col, val, labels, d)
    # no heavy columns: light-only path (with the sorted visit order)
    assert shard3.csc_heavy["task_idx"].numel() == 0
    g3, l3 = shard3.eval(w, 0)
    torch.testing.assert_close(gh, g3, rtol=1e-4, atol=1e-4)


def test_csc_grad_multi_skew_matches_oracle(monkeypatch):
    """Multiclass skew-robust CSC gradient vs the torch oracle on a skewed
    shard (k_csc_heavy_partial_multi / k_csc_heavy_combine_multi)."""
    from sparkagd_amd.data import CSRShard
    from sparkagd_amd.ops import multiclass as mc

    monkeypatch.setattr(CSRShard, "CSC_HEAVY_T", 128)
    monkeypatch.setattr(CSRShard, "CSC_TASK_S", 128)
    K = 6
    g = torch.Generator(device=DEV).manual_seed(19)
    n, d, nnz_per_row = 20000, 4000, 12
    nnz = n * nnz_per_row
    hot = torch.randint(0, 5, (nnz,), generator=g, device=DEV, dtype=torch.int32)
    uni = torch.randint(0, d, (nnz,), generator=g, device=DEV, dtype=torch.int32)
    pick = torch.rand(nnz, generator=g, device=DEV) < 0.35
    col = torch.where(pick, hot * 797 % d, uni).to(torch.int32)
    col = col.view(n, nnz_per_row).sort(dim=1).values.reshape(-1)
    val = torch.randn(nnz, generator=g, device=DEV)
    rowptr = torch.arange(0, nnz + 1, nnz_per_row, device=DEV, dtype=torch.int32)
    labels = torch.randint(0, K, (n,), generator=g, device=DEV).float()
    shard = CSRShard(rowptr, col, val, labels, d)
    assert shard.csc_heavy is not None

    from sparkagd_amd import MultinomialLogisticGradient

    W = (torch.randn(d * K, generator=g, device=DEV) / 4.0).contiguous()
    grad = MultinomialLogisticGradient(K)
    gh, lh = grad.eval(shard, W)
    zf = mc.ref_csr_margins_multi(shard.rowptr, shard.col, shard.val, W, K,
                                  d).reshape(-1, K)
    m, lr = mc.ref_multiplier_multi(zf, labels)
    gr = mc.ref_csr_grad_multi(shard.rowptr, shard.col, shard.val, m, d)
    torch.testing.assert_close(lh, lr, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(gh, gr, rtol=3e-4, atol=3e-4)
    gh2, lh2 = grad.eval(shard, W)
    assert torch.equal(gh, gh2)


def test_fuzz_dense_eval_random_configs():
    """Randomized parity sweep: dense eval (all 4 binary losses x dtypes x
    mask/weight combos x awkward shapes) vs the torch oracle. Seeded — the
    'random' configs are fixed, this is broad coverage, not flakiness."""
    from sparkagd_amd.ops import reference as ref

    g = torch.Generator(device=DEV).manual_seed(123)
    shapes = [(1023, 257), (4096, 1000), (777, 4096), (129, 16384)]
    dtypes = [torch.float32, torch.bfloat16]
    for li, loss_type in enumerate([0, 1, 2, 3]):
        n, d = shapes[li % len(shapes)]
        dt = dtypes[li % 2]
        A = (torch.randn((n, d), generator=g, device=DEV) / d ** 0.5).to(dt).contiguous()
        y = (torch.rand(n, generator=g, device=DEV) < 0.5).float()
        w = torch.randn(d, generator=g, device=DEV) * 0.1
        mask = (torch.rand(n, generator=g, device=DEV) < 0.8).to(torch.uint8)
        sw = torch.rand(n, generator=g, device=DEV) + 0.25
        for m_arg, w_arg in [(None, None), (mask, None), (mask, sw)]:
            from sparkagd_amd import ops as _ops

            gh, lh = _ops.dense_eval(A, y, w, loss_type, m_arg, True, w_arg)
            gr, lr = ref.dense_eval(A, y, w, loss_type, m_arg, True, w_arg)
            torch.testing.assert_close(lh, lr, rtol=5e-4, atol=5e-4)
            torch.testing.assert_close(gh, gr, rtol=5e-3, atol=5e-3)


def test_fuzz_csr_eval_random_configs():
    """Randomized CSR parity sweep incl. skewed columns, empty rows and
    duplicate column indices, vs the torch oracle."""
    from sparkagd_amd.data import CSRShard
    from sparkagd_amd.ops import reference as ref

    g = torch.Generator(device=DEV).manual_seed(321)
    for cfg in range(4):
        n = [5000, 1701, 12000, 300][cfg]
        d = [2000, 517, 30000, 40][cfg]
        nnz_row = [8, 3, 24, 5][cfg]
        # variable row lengths 0 .. 2*nnz_row (mean nnz_row); every seventh
        # row and the first and last are empty (rowptr[k] == rowptr[k+1])
        counts = torch.randint(0, 2 * nnz_row + 1, (n,), generator=g, device=DEV)
        counts[::7] = 0
        counts[-1] = 0
        rowptr = torch.zeros(n + 1, device=DEV, dtype=torch.int32)
        rowptr[1:] = torch.cumsum(counts, 0)
        nnz = int(rowptr[-1])
        rows = torch.repeat_interleave(torch.arange(n, device=DEV), counts)
        if cfg % 2 == 0:  # skewed: 30% of entries in a few hot columns
            hot = torch.randint(0, 3, (nnz,), generator=g, device=DEV)
            uni = torch.randint(0, d, (nnz,), generator=g, device=DEV)
            pick = torch.rand(nnz, generator=g, device=DEV) < 0.3
            col = torch.where(pick, hot * max(d // 7, 1) % d, uni).to(torch.int32)
        else:
            col = torch.randint(0, d, (nnz,), generator=g, device=DEV,
                                dtype=torch.int32)
        # columns ascending within each row (duplicates stay)
        col = (rows * d + col.to(torch.int64)).sort().values.remainder(d).to(torch.int32)
        val = torch.randn(nnz, generator=g, device=DEV)
        labels = (torch.rand(n, generator=g, device=DEV) < 0.5).float()
        shard = CSRShard(rowptr, col, val, labels, d)
        assert int((torch.diff(shard.rowptr) == 0).sum()) >= n // 7
        w = torch.randn(d, generator=g, device=DEV) * 0.1
        loss_type = cfg % 4
        gh, lh = shard.eval(w, loss_type)
        gr, lr = ref.csr_eval(shard.rowptr, shard.col, shard.val, labels, w,
                              loss_type, None, d)
        torch.testing.assert_close(lh, lr.to(lh.dtype), rtol=5e-4, atol=5e-4)
        torch.testing.assert_close(gh, gr.to(gh.dtype), rtol=5e-3, atol=5e-3)
        gh2, lh2 = shard.eval(w, loss_type)
        assert torch.equal(gh, gh2), "determinism must hold on every config"


def test_fuzz_multiclass_eval_random_configs():
    """Randomized multinomial parity sweep: eval_multi vs the torch oracle
    across K (VALU-templated and generic), dtypes and mask/weight combos."""
    from sparkagd_amd.ops import multiclass as mc

    g = torch.Generator(device=DEV).manual_seed(777)
    cases = [(5000, 333, 3, torch.float32), (4096, 512, 16, torch.bfloat16),
             (2048, 1024, 37, torch.bfloat16), (1000, 257, 64, torch.float32)]
    for n, d, K, dt in cases:
        A = (torch.randn((n, d), generator=g, device=DEV) / d ** 0.5).to(dt).contiguous()
        y = torch.randint(0, K, (n,), generator=g, device=DEV).float()
        W = (torch.randn(d * K, generator=g, device=DEV) * 0.2).contiguous()
        mask = (torch.rand(n, generator=g, device=DEV) < 0.75).to(torch.uint8)
        sw = torch.rand(n, generator=g, device=DEV) + 0.5
        for m_arg, w_arg in [(None, None), (mask, sw)]:
            gh, lh = mc.eval_multi(A, y, W, K, m_arg, True, w_arg)
            gr, lr = mc.ref_eval_multi(A.float(), y, W, K, m_arg, True, w_arg)
            torch.testing.assert_close(lh, lr, rtol=1e-4, atol=1e-4)
            torch.testing.assert_close(gh, gr, rtol=5e-3, atol=5e-3)
            gh2, lh2 = mc.eval_multi(A, y, W, K, m_arg, True, w_arg)
            assert torch.equal(gh, gh2) and torch.equal(lh, lh2)


def test_gemm_autotune_toggle_parity(tmp_path):
    """SPARKAGD_GEMM_TUNE=0 (the deterministic multi-rank pick) and the
    tuned default produce the same GEMM results within bf16-accumulation
    tolerance — the algo choice changes scheduling, not math. Checked via a
    subprocess because the knob is read once per process."""
    import os
    import subprocess
    import sys

    script = r"""
import sys, torch
sys.path.insert(0, %r)
from sparkagd_amd.ops import hiplib
g = torch.Generator(device="cuda:0").manual_seed(5)
A = (torch.randn((4096, 1024), generator=g, device="cuda:0") / 32).to(torch.bfloat16).contiguous()
B = (torch.randn((640, 1024), generator=g, device="cuda:0") / 32).to(torch.bfloat16).contiguous()
C = torch.empty((4096, 640), dtype=torch.float32, device="cuda:0")
hiplib.gemm_bf16f32_nt(A, B, C)
torch.save(C.cpu(), sys.argv[1])
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),)
    outs = {}
    for mode in ("0", "1"):
        env = dict(os.environ, SPARKAGD_GEMM_TUNE=mode)
        p = str(tmp_path / f"c{mode}.pt")
        r = subprocess.run([sys.executable, "-c", script, p], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[mode] = torch.load(p)
    torch.testing.assert_close(outs["0"], outs["1"], rtol=2e-3, atol=2e-3)
