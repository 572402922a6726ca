"""Native unpenalised intercept on CPU (f64 oracles): InterceptShard against
the ones-appended dense shard, the free-tail prox, the trainers' ``intercept``
option, the tracked-margin correction, the model plumbing, and gloo world 2."""

import math
import os

import pytest
import torch
import torch.multiprocessing as mp

from sparkagd_amd import (
    CSRShard,
    Communicator,
    DenseShard,
    ElasticNetUpdater,
    FreeTailUpdater,
    HostStreamedDenseShard,
    InterceptShard,
    L1Updater,
    LinearModel,
    LogisticGradient,
    LogisticRegressionWithAGD,
    LogisticRegressionWithSGD,
    MixedShard,
    MultinomialLogisticGradient,
    SimpleUpdater,
    SquaredL2Updater,
    evaluate,
    ops,
    regularization_path,
    run,
)
from sparkagd_amd.data import shard_range

F64 = torch.float64
LOSSES = [ops.LOSS_LOGISTIC, ops.LOSS_LEAST_SQUARES, ops.LOSS_HINGE,
          ops.LOSS_SMOOTH_HINGE]
KINDS = [ops.PROX_SIMPLE, ops.PROX_L1, ops.PROX_SQUARED_L2,
         ops.PROX_ELASTIC_NET]


def _problem(n, d, seed, bias=0.0, sparsity=0.0, scale=None):
    """Features [n, d] f64 (a fraction ``sparsity`` of entries zeroed),
    labels drawn from the planted logistic model with the given bias."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(n, d, generator=g, dtype=F64)
    if scale is not None:
        A = A * scale
    if sparsity > 0:
        A = A * (torch.rand(n, d, generator=g) >= sparsity).to(F64)
    w = torch.randn(d, generator=g, dtype=F64)
    y = (torch.rand(n, generator=g, dtype=F64)
         < torch.sigmoid(A @ w + bias)).to(F64)
    return A, y, w


def _csr(A, y, sw=None, deterministic=True):
    s = A.to_sparse_csr()
    return CSRShard(s.crow_indices(), s.col_indices(), s.values(), y,
                    A.shape[1], deterministic=deterministic, sample_weight=sw)


def _ones_appended(A, y, sw=None):
    return DenseShard(torch.cat([A, torch.ones(A.shape[0], 1, dtype=A.dtype)],
                                dim=1), y, sw)


def _make(kind, A, y, sw):
    if kind == "dense":
        return DenseShard(A, y, sw)
    if kind == "csr":
        return _csr(A, y, sw)
    k = 100  # two-part mixed: dense rows then CSR rows
    return MixedShard([
        DenseShard(A[:k], y[:k], None if sw is None else sw[:k]),
        _csr(A[k:], y[k:], None if sw is None else sw[k:])])


# --- 1. oracle equivalence -------------------------------------------------

@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("loss_type", LOSSES)
@pytest.mark.parametrize("kind", ["dense", "csr", "mixed"])
def test_intercept_shard_equals_ones_column(kind, loss_type, weighted):
    n, d = 257, 5
    A, y, _ = _problem(n, d, seed=3, sparsity=0.4)
    g = torch.Generator().manual_seed(11)
    sw = torch.rand(n, generator=g) * 2.0 if weighted else None
    mask = (torch.rand(n, generator=g) < 0.6).to(torch.uint8) if weighted else None
    wb = torch.randn(d + 1, generator=g, dtype=F64)

    sh = InterceptShard(_make(kind, A, y, sw))
    oracle = _ones_appended(A, y, sw)
    assert sh.kind == "intercept" and sh.d == d + 1 and sh.n == n
    assert sh.nbytes == sh.inner.nbytes

    tol = dict(rtol=1e-12, atol=1e-12)
    g1, lc1 = sh.eval(wb, loss_type, mask)
    g0, lc0 = oracle.eval(wb, loss_type, mask)
    assert g1.shape == (d + 1,)
    torch.testing.assert_close(g1, g0, **tol)
    torch.testing.assert_close(lc1, lc0, **tol)

    z1, z0 = sh.margins(wb), oracle.margins(wb)
    torch.testing.assert_close(z1, z0, **tol)
    none1, l1 = sh.eval_from_margins(z1, loss_type, mask, need_grad=False)
    none0, l0 = oracle.eval_from_margins(z0, loss_type, mask, need_grad=False)
    assert none1 is None and none0 is None
    torch.testing.assert_close(l1, l0, **tol)
    g2, l2 = sh.eval_from_margins(z1, loss_type, mask)
    torch.testing.assert_close(g2, g0, **tol)
    torch.testing.assert_close(l2, lc0, **tol)


# --- 2. prox(n_free=1) -----------------------------------------------------

@pytest.mark.parametrize("n", [2, 4, 5, 8, 9])
@pytest.mark.parametrize("kind", KINDS)
def test_prox_free_tail(kind, n):
    g = torch.Generator().manual_seed(n)
    w = torch.randn(n, generator=g, dtype=F64)
    gr = torch.randn(n, generator=g, dtype=F64)
    step, lam = 0.37, 0.21
    lam2 = 0.11 if kind == ops.PROX_ELASTIC_NET else 0.0
    out, reg = ops.prox(kind, w, gr, step, lam, lam2, n_free=1)
    head, reg_head = ops.prox(kind, w[:n - 1], gr[:n - 1], step, lam, lam2)
    assert out.shape == (n,)
    assert torch.equal(out[:n - 1], head)
    assert torch.equal(reg, reg_head)
    assert torch.equal(out[n - 1], w[n - 1] - step * gr[n - 1])
    # n_free=0 is the existing call
    out0, reg0 = ops.prox(kind, w, gr, step, lam, lam2, n_free=0)
    ref0, rreg0 = ops.prox(kind, w, gr, step, lam, lam2)
    assert torch.equal(out0, ref0) and torch.equal(reg0, rreg0)


def test_free_tail_updater_forwards_base():
    en = FreeTailUpdater(ElasticNetUpdater(0.3))
    assert en.n_free == 1 and en.AFFINE_PROX is False
    l2 = FreeTailUpdater(SquaredL2Updater())
    assert l2.AFFINE_PROX is True
    assert l2.prox_margin_coeffs(0.5, 0.2) == SquaredL2Updater().prox_margin_coeffs(0.5, 0.2)

    class _AffineNoCoeffs(SquaredL2Updater):  # prox_margins only
        def prox_margin_coeffs(self, step, reg_param):
            raise NotImplementedError

    # no (pz, pg) form -> no place for the free-coordinate correction:
    # such a base must run untracked
    assert FreeTailUpdater(_AffineNoCoeffs()).AFFINE_PROX is False
    assert FreeTailUpdater(SquaredL2Updater(), n_free=2).AFFINE_PROX is False
    w = torch.tensor([1.0, -2.0, 3.0], dtype=F64)
    g = torch.tensor([0.5, 0.25, -1.0], dtype=F64)
    out, reg = en.compute(w, g, 0.4, 4, 0.5)  # step 0.4 / sqrt(4)
    head, rh = ElasticNetUpdater(0.3).compute(w[:2], g[:2], 0.4, 4, 0.5)
    assert torch.equal(out[:2], head) and torch.equal(reg, rh)
    assert float(out[2]) == 3.0 + 0.2
    assert torch.equal(en.reg_value(w, 0.5),
                       ElasticNetUpdater(0.3).reg_value(w[:2], 0.5))


# --- 3. unregularised training ---------------------------------------------

def test_unregularised_training_matches_ones_column():
    A, y, _ = _problem(300, 5, seed=5, bias=1.0)
    m = LogisticRegressionWithAGD.train(DenseShard(A, y), intercept=True,
                                        reg_param=0, num_iterations=15)
    ref = LogisticRegressionWithAGD.train(_ones_appended(A, y),
                                          updater=SimpleUpdater(),
                                          reg_param=0, num_iterations=15)
    assert len(m.loss_history) == len(ref.loss_history) == 15
    torch.testing.assert_close(torch.tensor(m.loss_history),
                               torch.tensor(ref.loss_history),
                               rtol=1e-10, atol=0)
    assert m.weights.shape == (5,)
    torch.testing.assert_close(m.weights, ref.weights[:5], rtol=1e-8, atol=1e-10)
    assert m.intercept == pytest.approx(float(ref.weights[5]), rel=1e-8)


# --- 4. the bias is not penalised ------------------------------------------

def _objective_l2(A, y, wb, lam):
    """mean logistic loss + lam/2 * ||w||^2, the bias wb[-1] free."""
    z = A @ wb[:-1] + wb[-1]
    terms = torch.where(y > 0, torch.nn.functional.softplus(-z),
                        torch.nn.functional.softplus(z))
    # exactly rounded sums: the gap below is compared at the ulp level
    return (math.fsum(terms.tolist()) / terms.numel()
            + 0.5 * lam * math.fsum((wb[:-1] ** 2).tolist()))


def _newton_l2_free_bias(A, y, lam, iters=50):
    """Independent f64 Newton solve of the free-bias L2 objective."""
    n, d = A.shape
    X = torch.cat([A, torch.ones(n, 1, dtype=F64)], dim=1)
    pen = torch.cat([torch.full((d,), lam, dtype=F64), torch.zeros(1, dtype=F64)])
    wb = torch.zeros(d + 1, dtype=F64)
    for _ in range(iters):
        p = torch.sigmoid(X @ wb)
        grad = X.T @ (p - y) / n + pen * wb
        H = (X.T * (p * (1 - p))) @ X / n + torch.diag(pen)
        wb = wb - torch.linalg.solve(H, grad)
    assert float(grad.norm()) < 1e-12
    return wb


def test_l2_does_not_penalise_bias():
    n, d, lam = 400, 5, 0.1
    A, y, _ = _problem(n, d, seed=21, bias=2.0)
    star = _newton_l2_free_bias(A, y, lam)
    f_star = _objective_l2(A, y, star, lam)

    m = LogisticRegressionWithAGD.train(
        DenseShard(A, y), intercept=True, updater=SquaredL2Updater(),
        reg_param=lam, convergence_tol=1e-10, num_iterations=2000)
    wb = torch.cat([m.weights, torch.tensor([m.intercept], dtype=F64)])
    gap = _objective_l2(A, y, wb, lam) - f_star
    print(f"free-bias AGD objective gap {gap:.3e} (f* = {f_star:.6f}, "
          f"{len(m.loss_history)} iterations, "
          f"|wb - w*| = {float((wb - star).norm()):.3e})")
    # Measured: AGD stops after 47 iterations at |wb - w*| = 2.3e-10, where
    # the true gap (~ |wb - w*|^2) is far below what f64 can resolve: the
    # computed gap is 0.0, i.e. within one ulp of f* = 0.4658, 5.6e-17. That
    # resolution is the measured value; the bound is 10x it, and never
    # looser than 1e-6 relative.
    bound = min(10 * MEASURED_L2_GAP, 1e-6 * f_star)
    assert abs(gap) < bound, (gap, bound)
    # The distance to the optimum is a quantity f64 does resolve: measured
    # 2.3e-10 (convergence_tol = 1e-10 on |dx| / |x|); bound 10x that.
    dist = float((wb - star).norm())
    dist_bound = 10 * MEASURED_L2_DIST
    assert dist < dist_bound, (dist, dist_bound)

    # the penalised ones-column route solves another problem: under the
    # free-bias objective it is far outside the bound
    pen = LogisticRegressionWithAGD.train(
        _ones_appended(A, y), updater=SquaredL2Updater(), reg_param=lam,
        convergence_tol=1e-10, num_iterations=2000)
    gap_pen = _objective_l2(A, y, pen.weights, lam) - f_star
    print(f"penalised ones-column objective gap {gap_pen:.3e}")
    assert gap_pen >= 100 * bound, (gap_pen, bound)
    dist_pen = float((pen.weights - star).norm())
    print(f"penalised ones-column |wb - w*| = {dist_pen:.3e}")
    assert dist_pen >= 100 * dist_bound, (dist_pen, dist_bound)
    assert abs(float(pen.weights[-1])) < abs(m.intercept)


#: objective gap of the converged free-bias AGD solution to the Newton optimum
#: in test_l2_does_not_penalise_bias (f64, n=400, d=5, lam=0.1): zero to
#: within one ulp of f* = 0.4658
MEASURED_L2_GAP = 5.6e-17
#: |wb - w*| of the same solution
MEASURED_L2_DIST = 2.3e-10


def test_l1_does_not_threshold_bias():
    """Small true bias, strong L1: the penalised ones column is
    soft-thresholded to exactly zero, the free bias is fitted."""
    n, d, lam = 400, 5, 0.05
    A, y, _ = _problem(n, d, seed=22, bias=0.15)
    pen = LogisticRegressionWithAGD.train(
        _ones_appended(A, y), updater=L1Updater(), reg_param=lam,
        convergence_tol=1e-10, num_iterations=500)
    assert float(pen.weights[-1]) == 0.0
    m = LogisticRegressionWithAGD.train(
        DenseShard(A, y), intercept=True, updater=L1Updater(), reg_param=lam,
        convergence_tol=1e-10, num_iterations=500)
    assert abs(m.intercept) > 0.02
    # first-order optimality of a free coordinate: sum of multipliers is zero
    z = A @ m.weights + m.intercept
    assert abs(float((torch.sigmoid(z) - y).mean())) < 1e-6


# --- 5. tracked equals untracked -------------------------------------------

class _Rec:
    def __init__(self):
        self.rows = []

    def log(self, **kw):
        self.rows.append(kw)


def _tracked_vs_untracked(A, y, iters=12, may_restart=True,
                          margin_refresh_every=0, w0_scale=0.0):
    sh = InterceptShard(DenseShard(A, y))
    upd = FreeTailUpdater(SquaredL2Updater())
    w0 = w0_scale * torch.randn(sh.d, dtype=F64,
                                generator=torch.Generator().manual_seed(1))
    recs = []
    outs = []
    for track in (True, False):
        rec = _Rec()
        outs.append(run(sh, LogisticGradient(), upd, 1e-14, iters, 0.05, w0,
                        1.0, math.inf, 0.5, 0.9, may_restart,
                        track_margins=track, metrics=rec,
                        margin_refresh_every=margin_refresh_every))
        recs.append(rec)
    (w_t, h_t), (w_u, h_u) = outs
    assert len(h_t) == len(h_u) == iters
    torch.testing.assert_close(torch.tensor(h_t), torch.tensor(h_u),
                               rtol=1e-9, atol=0)
    torch.testing.assert_close(w_t, w_u, rtol=1e-8, atol=1e-8)
    return recs[0]


def test_tracked_equals_untracked():
    A, y, _ = _problem(300, 5, seed=31, bias=1.5)
    _tracked_vs_untracked(A, y, may_restart=False)


def test_tracked_equals_untracked_with_restart_and_refresh():
    # a start far from the optimum makes the momentum overshoot: the
    # gradient test restarts from iteration 6 on
    A, y, _ = _problem(300, 5, seed=39, bias=1.5)
    rec = _tracked_vs_untracked(A, y, may_restart=True, w0_scale=3.0)
    restarts = [i for i, r in enumerate(rec.rows, 1) if r["restarted"]]
    assert restarts and restarts[0] < 12, "data must trigger a restart"
    _tracked_vs_untracked(A, y, may_restart=True, w0_scale=3.0,
                          margin_refresh_every=3)


def test_tracked_offset_is_needed():
    """Without the (1 - pz)*z_b term the tracked margins drift from the
    weights: the plain update differs from the corrected one."""
    z = torch.tensor([0.5, -1.0, 2.0], dtype=F64)  # [w; b]
    zm = torch.randn(7, dtype=F64)
    gm = torch.randn(7, dtype=F64)
    zn, xn = ops.at_margin_update(zm, zm, gm, 0.9, -0.5, 0.3,
                                  offset=(0.1, z, 2))
    z0, x0 = ops.at_margin_update(zm, zm, gm, 0.9, -0.5, 0.3)
    torch.testing.assert_close(zn, z0 + 0.2, rtol=1e-14, atol=1e-14)
    torch.testing.assert_close(xn, x0 + 0.3 * 0.2, rtol=1e-14, atol=1e-14)


# --- 6. scaling and the model ----------------------------------------------

def test_scaling_and_model_plumbing(tmp_path):
    from sparkagd_amd import StandardScaler

    col_scale = torch.tensor([1.0, 10.0, 0.1, 3.0, 0.5], dtype=F64)
    A, y, _ = _problem(300, 5, seed=41, bias=-1.0, scale=col_scale)
    sh = DenseShard(A, y)
    m = LogisticRegressionWithAGD.train(sh, feature_scaling=True,
                                        intercept=True, reg_param=0.01,
                                        num_iterations=30)
    assert m.weights.shape == (5,) and m.intercept != 0.0
    # raw-feature predictions == scaled features . scaled weights + b
    scaler = StandardScaler().fit(sh)
    scaled = scaler.transform(sh)
    w_scaled = scaler.scale_weights(m.weights)
    torch.testing.assert_close(m.margins(A),
                               scaled.features @ w_scaled + m.intercept,
                               rtol=1e-10, atol=1e-12)
    # shard scoring sees the bias
    torch.testing.assert_close(m.score(sh), m.margins(A), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(m.predict_shard(sh), m.predict(A))
    torch.testing.assert_close(m.predict_proba(A), torch.sigmoid(m.margins(A)))
    no_bias = LinearModel(m.weights, m.loss_history, m.link)
    assert no_bias.intercept == 0.0
    torch.testing.assert_close(m.margins(A) - m.intercept, no_bias.margins(A),
                               rtol=1e-12, atol=1e-12)
    assert evaluate(m, sh).log_loss != evaluate(no_bias, sh).log_loss
    assert evaluate(m, sh).log_loss < evaluate(no_bias, sh).log_loss

    # save / load round trip, and a file written without the field
    p = str(tmp_path / "m.safetensors")
    m.save(p)
    back = LinearModel.load(p)
    assert back.intercept == m.intercept and torch.equal(back.weights, m.weights)
    from sparkagd_amd.models.trainers import _save_model

    old = str(tmp_path / "old.safetensors")
    _save_model(old, m.weights, {"kind": "linear", "link": "logistic",
                                 "loss_history": []})
    assert LinearModel.load(old).intercept == 0.0


def test_intercept_false_is_the_default_path():
    A, y, _ = _problem(200, 5, seed=42)
    sh = DenseShard(A, y)
    a = LogisticRegressionWithAGD.train(sh, num_iterations=8, reg_param=0.1)
    b = LogisticRegressionWithAGD.train(sh, num_iterations=8, reg_param=0.1,
                                        intercept=False)
    assert torch.equal(a.weights, b.weights)
    assert a.loss_history == b.loss_history and b.intercept == 0.0
    c = LogisticRegressionWithSGD.train(sh, num_iterations=8)
    e = LogisticRegressionWithSGD.train(sh, num_iterations=8, intercept=False)
    assert torch.equal(c.weights, e.weights) and c.loss_history == e.loss_history


def test_sgd_and_path_fit_a_bias():
    A, y, _ = _problem(400, 5, seed=43, bias=1.5)
    sh = DenseShard(A, y)
    s = LogisticRegressionWithSGD.train(sh, num_iterations=60, intercept=True,
                                        mini_batch_fraction=0.5, reg_param=0.01,
                                        initial_intercept=0.5)
    assert s.weights.shape == (5,) and s.intercept > 0.5
    models = regularization_path(sh, [1.0, 0.1], intercept=True,
                                 num_iterations=40)
    assert all(m.weights.shape == (5,) and m.intercept > 0.5 for m in models)
    with pytest.raises(ValueError, match="direct solver"):
        regularization_path(sh, [1.0], intercept=True, solver="gram")


# --- 7. errors ---------------------------------------------------------------

def test_unsupported_combinations_raise():
    A, y, _ = _problem(64, 4, seed=51)
    with pytest.raises(NotImplementedError, match="HostStreamedDenseShard"):
        InterceptShard(HostStreamedDenseShard(A, y, device="cpu", chunk_rows=16))
    sh = InterceptShard(DenseShard(A, y))
    with pytest.raises(ValueError, match="already"):
        InterceptShard(sh)
    mg = MultinomialLogisticGradient(3)
    with pytest.raises(ValueError, match="InterceptShard"):
        mg.eval(sh, torch.zeros(sh.d * 3, dtype=F64))
    with pytest.raises(ValueError, match="InterceptShard"):
        mg.margins(sh, torch.zeros(sh.d * 3, dtype=F64))
    w0 = torch.zeros(sh.d, dtype=F64)
    with pytest.raises(ValueError, match="Gram solver"):
        run(sh, LogisticGradient(), FreeTailUpdater(SquaredL2Updater()), 1e-6,
            3, 0.1, w0, solver="gram")
    from sparkagd_amd import GramOperator

    with pytest.raises(ValueError, match="Gram solver"):
        GramOperator(sh, Communicator())
    with pytest.raises(ValueError, match="length"):
        sh.margins(torch.zeros(sh.d - 1, dtype=F64))


# --- 8. gloo world 2 ---------------------------------------------------------

N_DIST = 600


def _dist_shard(lo, hi):
    A, y, _ = _problem(N_DIST, 5, seed=61, bias=1.0, sparsity=0.3)
    return _csr(A[lo:hi], y[lo:hi])


def _dist_train(comm=None, lo=0, hi=N_DIST):
    m = LogisticRegressionWithAGD.train(
        _dist_shard(lo, hi), intercept=True, reg_param=0.05,
        num_iterations=15, comm=comm)
    return torch.cat([m.weights, torch.tensor([m.intercept], dtype=F64)])


def _dist_worker(rank, world, init_file, out_q):
    torch.distributed.init_process_group(
        "gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    try:
        lo, hi = shard_range(N_DIST, rank, world)
        out_q.put((rank, _dist_train(Communicator(), lo, hi)))
    except Exception:  # noqa: BLE001 - reported to the parent, which fails
        import traceback

        out_q.put((rank, traceback.format_exc()))
    finally:
        torch.distributed.destroy_process_group()


def _spawn_world(world):
    """One-shot gloo tier: ``world`` spawned processes, FileStore rendezvous,
    results gathered through a queue."""
    import tempfile

    fd, init_file = tempfile.mkstemp(prefix="sparkagd_icpt_", suffix=".init")
    os.close(fd)
    os.unlink(init_file)
    ctx = mp.get_context("spawn")
    out_q = ctx.Queue()
    procs = [ctx.Process(target=_dist_worker,
                         args=(r, world, init_file, out_q), daemon=True)
             for r in range(world)]
    for p in procs:
        p.start()
    try:
        results = dict(out_q.get(timeout=120) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=30)
    for rank, res in results.items():
        assert torch.is_tensor(res), f"rank {rank} failed:\n{res}"
    return results


def test_intercept_world2_matches_world1():
    res = _spawn_world(2)
    assert torch.equal(res[0], res[1]), "ranks must hold identical [w; b]"
    single = _dist_train()
    torch.testing.assert_close(res[0], single, rtol=1e-9, atol=1e-12)
