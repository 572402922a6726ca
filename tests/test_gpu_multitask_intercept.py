"""The per-task bias kernels (agd_tasks_bias.hip) against plain f64 oracles at
their tail shapes, and one-vs-rest / CV runs with intercepts on the GPU
against the CPU f64 run of the same problem."""

import functools
import math

import pytest
import torch

from sparkagd_amd import (
    AGDConfig, CSRShard, DenseShard, LogisticGradient, MultiTaskGradient,
    OneVsRestWithAGD, PerTaskUpdater, SquaredL2Updater, assign_folds,
    cross_validate, generate_dense_problem, run,
)
from sparkagd_amd.data import generate_csr_problem
from sparkagd_amd.ops import multitask as mt
from sparkagd_amd.ops.multiclass import padded_k

from test_multitask_tracked import _Record

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# every KC template with and without pads, the first any-KC width and one
# past a 256-column chunk
R_KC = [(3, 4), (8, 8), (15, 16), (32, 32), (33, 36), (257, 260)]
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64],
                                 ids=["f32", "f64"])
STEP, THETA = 0.37, 0.61


def _gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * 7919 ** i
                                             for i, s in enumerate(seed)))


# --- k_colsum_multi ---

# n = 300 001 at KC = 4: more 4-column groups than the 1024 x 256 grid holds
@pytest.mark.parametrize("r,kc,n", [(r, kc, n) for r, kc in R_KC
                                    for n in (1, 63, 1027)] + [(3, 4, 300_001)])
def test_colsum_multi_is_exact_on_small_integers(r, kc, n):
    assert padded_k(r) == kc
    M = torch.randint(-2, 3, (n, kc), generator=_gen(r, n)).float()
    want = M.double().sum(0)[:r]
    for tdt in (torch.float32, torch.float64):
        grad = torch.full((5 + r,), 9.0, dtype=tdt, device=DEV)
        got = mt.colsum_multi(M.reshape(-1).to(DEV), r, tail=grad[5:])
        assert got.dtype == torch.float64
        assert torch.equal(got.cpu(), want)
        assert torch.equal(grad[5:].cpu(), want.to(tdt))
        assert torch.equal(grad[:5].cpu(), torch.full((5,), 9.0, dtype=tdt))


@pytest.mark.parametrize("r,n", [(15, 70_001), (33, 5000)])
def test_colsum_multi_is_bitwise_repeatable(r, n):
    M = torch.randn(n * padded_k(r), generator=_gen(r, n)).to(DEV)
    a, b = mt.colsum_multi(M, r), mt.colsum_multi(M, r)
    assert torch.equal(a, b)
    want = M.reshape(n, -1).double().sum(0)[:r]
    torch.testing.assert_close(a, want, rtol=1e-12, atol=1e-9)


# --- k_add_bias_cols ---

@DTYPES
@pytest.mark.parametrize("coef", [1.0, -0.5])
@pytest.mark.parametrize("n", [1, 1027])
@pytest.mark.parametrize("r,kc", R_KC)
def test_add_bias_cols_is_exact_on_dyadic_data(r, kc, n, coef, dtype):
    g = _gen(r, n)
    Z = (torch.randint(-64, 65, (n, kc), generator=g) / 4.0).to(dtype)
    if kc > r:  # pads must come back bit for bit: -0.0 and NaN included
        Z[:, r:] = torch.tensor([-0.0, float("nan"), 7.0])[
            torch.randint(0, 3, (n, kc - r), generator=g)].to(dtype)
    src = (torch.randint(-64, 65, (11 + r,), generator=g) / 8.0).to(dtype)
    want = mt.ref_add_bias_cols(Z.clone().reshape(-1), coef, src, 11, r)
    zd = Z.reshape(-1).to(DEV)
    got = mt.add_bias_cols(zd, coef, src.to(DEV), 11, r)
    assert got.data_ptr() == zd.data_ptr()
    bits = torch.int32 if dtype == torch.float32 else torch.int64
    got2, want2 = got.cpu().reshape(n, kc), want.reshape(n, kc)
    assert torch.equal(got2[:, :r], want2[:, :r])
    assert torch.equal(got2[:, r:].contiguous().view(bits),
                       Z[:, r:].contiguous().view(bits))


# --- k_at_margin_update_tasks_off ---

@functools.lru_cache(maxsize=None)
def _update_inputs(n, r, dtype, pad_fill):
    g = _gen(n, r)
    kc = padded_k(r)
    flats = []
    for _ in range(3):
        t = torch.randn(n, kc, generator=g, dtype=dtype)
        t[:, r:] = pad_fill
        flats.append(t.reshape(-1))
    lam = torch.rand(r, generator=g, dtype=torch.float64)
    z_old = torch.randn(20 + r, generator=g, dtype=dtype)
    return flats, lam, z_old


@DTYPES
@pytest.mark.parametrize("n", [1, 1027])
@pytest.mark.parametrize("r,kc", R_KC)
def test_at_margin_update_offset_matches_f64_oracle(r, kc, n, dtype):
    (zm, xm, gm), lam, z_old = _update_inputs(n, r, dtype, float("nan"))
    zn, xn = mt.at_margin_update_tasks(
        zm.to(DEV), xm.to(DEV), gm.to(DEV), STEP, lam.to(DEV), THETA, r,
        offset=(z_old.to(DEV), 20))
    zn, xn = zn.cpu().reshape(n, kc), xn.cpu().reshape(n, kc)
    # NaN planted in the pads of every input: exact-zero pads come out
    assert torch.equal(zn[:, r:], torch.zeros(n, kc - r, dtype=dtype))
    assert torch.equal(xn[:, r:], torch.zeros(n, kc - r, dtype=dtype))
    # the f64 value of the kernel's own (cast) coefficients
    c = lambda v: torch.as_tensor(v, dtype=torch.float64).to(dtype).double()
    pz64 = 1.0 - STEP * lam
    pz, omp, st, th, om = c(pz64), c(1.0 - pz64), c(STEP), c(THETA), c(1.0 - THETA)
    Z, X, G = (t.reshape(n, kc)[:, :r].double() for t in (zm, xm, gm))
    zb = z_old[20:].double()
    z_ref = pz * Z - st * G + omp * zb
    x_ref = om * X + th * z_ref
    if dtype == torch.float64:
        bound = torch.full_like(Z, 1e-12)
    else:  # three roundings for zm', two more for xm'
        bound = 4.0 * 2.0 ** -24 * ((pz * Z).abs() + (st * G).abs()
                                    + (omp * zb).abs().expand_as(Z) + X.abs())
    for got, want in ((zn, z_ref), (xn, x_ref)):
        err = (got[:, :r].double() - want).abs()
        print(f"worst error / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())


@DTYPES
@pytest.mark.parametrize("r,kc", R_KC)
def test_at_margin_update_zero_bias_is_bitwise_the_plain_kernel(r, kc, dtype):
    (zm, xm, gm), lam, z_old = _update_inputs(1027, r, dtype, 7.0)
    dev = [t.to(DEV) for t in (zm, xm, gm)]
    plain = mt.at_margin_update_tasks(*dev, STEP, lam.to(DEV), THETA, r)
    off = mt.at_margin_update_tasks(*dev, STEP, lam.to(DEV), THETA, r,
                                    offset=(torch.zeros_like(z_old).to(DEV), 20))
    assert torch.equal(off[0], plain[0]) and torch.equal(off[1], plain[1])


# --- k_prox_tasks_free ---

# the bias row starts inside the 16-B body, straddles body and scalar tail,
# is vector-aligned, and is wider than a vector row
@DTYPES
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("d,r", [(5, 3), (7, 15), (4, 4), (3, 33)])
def test_prox_tasks_free_row(d, r, kind, dtype):
    g = _gen(d, r, kind)
    w = torch.randn((d + 1) * r, generator=g, dtype=dtype).to(DEV)
    grad = torch.randn((d + 1) * r, generator=g, dtype=dtype).to(DEV)
    lam = torch.rand(r, generator=g, dtype=torch.float64).to(DEV)
    lam2 = torch.rand(r, generator=g, dtype=torch.float64).to(DEV)
    out, reg = mt.prox_tasks(kind, w, grad, STEP, lam, lam2, n_free=r)
    head, reg_head = mt.prox_tasks(kind, w[:d * r], grad[:d * r], STEP, lam, lam2)
    assert out.dtype == dtype
    assert torch.equal(out[:d * r], head)
    assert torch.equal(out[d * r:], w[d * r:] - STEP * grad[d * r:])
    # the same <= 99 f64 terms in another order
    torch.testing.assert_close(reg, reg_head, rtol=1e-13, atol=0.0)


# --- solver: GPU runs with intercepts against the CPU f64 run ---

N, D, K, ITERS = 2048, 256, 3, 25


def _class_labels(n):
    u = torch.rand(n, generator=_gen(n))
    return (u > 0.7).float() + (u > 0.9).float()  # 70 / 20 / 10 %


@functools.lru_cache(maxsize=None)
def _pair(kind, binary=False):
    """(CPU f64 shard, GPU shard, config) of the shapes the no-intercept
    comparisons use (test_gpu_multitask_tracked.py)."""
    y = _class_labels(N)
    if binary:
        y = (y > 0).float()
    if kind == "csr":
        src, _ = generate_csr_problem(n=N, d=D, nnz_per_row=8, seed=0)
        frob = float(src.val.double().norm() ** 2)
        cpu = CSRShard(src.rowptr, src.col, src.val.double(), y, src.d)
        gpu = CSRShard(src.rowptr.to(DEV), src.col.to(DEV), src.val.to(DEV),
                       y.to(DEV), src.d)
    else:
        dt = torch.bfloat16 if kind == "bf16" else torch.float32
        src, _ = generate_dense_problem(n=N, d=D, seed=0, dtype=dt)
        frob = float(src.features.double().norm() ** 2)
        cpu = DenseShard(src.features.double(), y)
        gpu = DenseShard(src.features.to(DEV), y.to(DEV))
    # that suite's L0 with the ones column counted in |A|_F^2
    L0 = 2.0 * (frob + N) / (N * 140.0 / 240.0) + 1.0
    return cpu, gpu, AGDConfig(L0=L0, beta=1.0, alpha=1.0, may_restart=False)


def _assert_matches_cpu(kind, hc, hg, wc, wg):
    wg = wg.double().cpu()
    assert len(hc) == len(hg) == ITERS
    if kind == "bf16":  # test_tracked_run_bf16_matches_cpu's
        for a, b in zip(hc, hg):
            assert abs(a - b) < 2e-3 * max(1.0, abs(a)), (a, b)
        assert float((wg - wc).norm() / wc.norm()) < 1e-2
    else:  # test_tracked_run_f32_dense / csr_matches_cpu's
        assert abs(hc[-1] - hg[-1]) <= 1e-3 * abs(hc[-1])
        torch.testing.assert_close(wg, wc, rtol=5e-3, atol=5e-3)


@functools.lru_cache(maxsize=None)
def _ovr(kind, where, intercept=True, track="auto"):
    cpu, gpu, cfg = _pair(kind)
    cfg = AGDConfig(L0=cfg.L0, beta=1.0, alpha=1.0, may_restart=False,
                    track_margins=track)
    return OneVsRestWithAGD.train(cpu if where == "cpu" else gpu, K,
                                  num_iterations=ITERS, reg_param=0.01,
                                  convergence_tol=0.0, config=cfg,
                                  intercept=intercept)


@pytest.mark.parametrize("kind", ["f32", "bf16", "csr"])
def test_one_vs_rest_intercept_matches_cpu(kind):
    mc_, mg = _ovr(kind, "cpu"), _ovr(kind, "gpu")
    full = lambda m: torch.cat([m.weights.reshape(-1).double().cpu(),
                                m.intercepts.double().cpu()])
    _assert_matches_cpu(kind, mc_.loss_history, mg.loss_history, full(mc_), full(mg))
    assert bool((mg.intercepts != 0).all())
    assert mg.loss_history[-1] < _ovr(kind, "gpu", intercept=False).loss_history[-1]
    # score() adds the intercepts to the margins of the same weights
    _, gpu, _ = _pair(kind)
    z, z0 = mg.score(gpu), type(mg)(mg.weights, [], K, mg.link).score(gpu)
    torch.testing.assert_close(z - z0, mg.intercepts.to(z.dtype).expand_as(z),
                               rtol=1e-5, atol=1e-5)


def test_one_vs_rest_intercept_tracked_matches_untracked():
    a, b = _ovr("f32", "gpu"), _ovr("f32", "gpu", track=False)
    # both are f32 runs of the same steps; the CPU comparison's tolerance
    assert abs(a.loss_history[-1] - b.loss_history[-1]) <= 1e-3 * abs(b.loss_history[-1])
    torch.testing.assert_close(a.weights, b.weights, rtol=5e-3, atol=5e-3)
    torch.testing.assert_close(a.intercepts, b.intercepts, rtol=5e-3, atol=5e-3)


@pytest.mark.parametrize("kind", ["f32", "bf16", "csr"])
def test_cv_sweep_intercept_matches_cpu(kind):
    cpu, gpu, cfg = _pair(kind, binary=True)
    folds = assign_folds(N, 2, seed=1)
    res = [cross_validate(s, [0.003, 0.03], n_folds=2, num_iterations=ITERS,
                          convergence_tol=0.0, fold_id=folds, refit=False,
                          intercept=True,
                          config=AGDConfig(L0=cfg.L0, beta=1.0, alpha=1.0,
                                           may_restart=False,
                                           track_margins=True))
           for s in (cpu, gpu)]
    full = lambda r: torch.cat([r.fold_weights.reshape(-1).double().cpu(),
                                r.fold_intercepts.reshape(-1).double().cpu()])
    _assert_matches_cpu(kind, res[0].loss_history, res[1].loss_history,
                        full(res[0]), full(res[1]))
    assert bool((res[1].fold_intercepts != 0).all())
    tol = 2e-3 if kind == "bf16" else 1e-3  # mean losses: the history's
    torch.testing.assert_close(res[1].heldout_loss, res[0].heldout_loss,
                               rtol=tol, atol=tol)


def test_intercept_adds_no_host_fetch():
    _, gpu, cfg = _pair("f32")
    fetches = []
    for b in (False, True):
        rec = _Record()
        grad = MultiTaskGradient(LogisticGradient(), K, target_class=range(K),
                                 intercept=b)
        run(gpu, grad, PerTaskUpdater(SquaredL2Updater(), [0.01] * K, free_rows=int(b)),
            0.0, 5, 1.0, torch.zeros((D + b) * K, dtype=torch.float32, device=DEV),
            cfg.L0, math.inf, 0.5, 0.9, True, metrics=rec)
        fetches.append([row["host_fetches"] for row in rec.rows])
    assert fetches[0] == fetches[1] and len(fetches[0]) == 5
