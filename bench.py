#!/usr/bin/env python3
"""Flagship benchmark: distributed accelerated gradient descent on dense
logistic regression, d = 10^6, bf16 shards, one process per MI355X over RCCL.

Driver contract:
    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
(for N > 1 the driver launches this under torch.distributed.run, one rank per
GPU; RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* come from the env). W untimed warmup
AGD iterations, then EXACTLY K timed iterations bracketed by a barrier +
torch.cuda.synchronize() on both sides; elapsed is the MAX over ranks; rank 0
prints ONE JSON line.

A plain run does only what the headline figure needs: set up, warm up, time
the K steps, write the outputs if --dump-outputs is given, print the line.
--full adds the second half of the metric: an untimed convergence run that
estimates L* and reports iters-to-eps (config.iters_to_eps / loss_star).
--dump-outputs DIR writes what the timed run returned to its caller
(DIR/weights.npy, DIR/loss_history.npy); the inputs are seeded, so two builds
can be compared output for output.

Metric: examples/sec — loss/gradient evaluations x rows per second,
aggregated over all ranks. Each AGD iteration performs 2 evaluations (at y,
and the accepted backtracking trial at x; the reference's third
TFOCS-validation pass, AGD.scala:302-307, is off — loss history reuses the
accepted f_x) over 2 physical shard streams (margin-state tracking;
config.data_passes_per_step reports the honest pass count). Weak scaling:
rows-per-GPU fixed as N grows.
"""

from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sparkagd_amd import (  # noqa: E402
    AGDConfig,
    LogisticGradient,
    LeastSquaresGradient,
    HingeGradient,
    MultinomialLogisticGradient,
    SimpleUpdater,
    SquaredL2Updater,
    generate_dense_problem,
    run,
)
from sparkagd_amd import ops  # noqa: E402
from sparkagd_amd.data import generate_csr_problem  # noqa: E402
from sparkagd_amd.models.gradient import SmoothedHingeGradient  # noqa: E402
from sparkagd_amd.parallel.comm import init_from_env  # noqa: E402
from sparkagd_amd.utils.metrics import iters_to_eps as _iters_to_eps  # noqa: E402

BASELINE_METRIC = "examples/sec + iters-to-ε, logistic regression d=10^6 at 1/2/4/8 MI355X"

# --loss hinge maps to the SMOOTHED hinge under AGD: the plain hinge is
# nonsmooth and the accelerated method's backtracking assumes a Lipschitz
# gradient (the reference cites TFOCS' smooth-f assumption,
# AGD.scala:154-157). hinge_plain keeps the exact MLlib HingeGradient
# semantics for parity runs.
LOSSES = {
    "logistic": (ops.LOSS_LOGISTIC, LogisticGradient),
    "lsq": (ops.LOSS_LEAST_SQUARES, LeastSquaresGradient),
    "hinge": (ops.LOSS_SMOOTH_HINGE, SmoothedHingeGradient),
    "hinge_plain": (ops.LOSS_HINGE, HingeGradient),
}


class CountingGradient:
    def __init__(self, inner):
        self.inner = inner
        self.n_evals = 0   # loss evaluations (each touches every example)
        self.n_passes = 0  # full data passes (grad eval = 2: A·w and A^T·m)

    def eval(self, shard, w, mask=None, need_grad=True):
        self.n_evals += 1
        self.n_passes += 2 if need_grad else 1
        return self.inner.eval(shard, w, mask, need_grad)

    def margins(self, shard, v):
        self.n_passes += 1
        return self.inner.margins(shard, v)

    def eval_from_margins(self, shard, margins, mask=None, need_grad=True):
        self.n_evals += 1
        self.n_passes += 1 if need_grad else 0
        return self.inner.eval_from_margins(shard, margins, mask, need_grad)

    def multiplier_loss(self, shard, margins, mask=None):
        self.n_evals += 1  # a loss evaluation over every example (n-space)
        return self.inner.multiplier_loss(shard, margins, mask)

    def count_eval(self, n: int = 1):
        """Called by fused solver paths that bypass the wrapped methods
        (gram.py fused trials): n loss evaluations, zero data passes."""
        self.n_evals += n

    @property
    def LOSS_TYPE(self):
        return self.inner.LOSS_TYPE

    @property
    def IS_MULTICLASS(self):
        return getattr(self.inner, "IS_MULTICLASS", False)

    @property
    def num_classes(self):
        return self.inner.num_classes


def sync(device: torch.device) -> None:
    if device.type == "cuda":
        torch.cuda.synchronize(device)


DUMP_BUDGET_BYTES = 64 * 2**20  # --dump-outputs writes at most this much


def dump_outputs(out_dir: str, weights: torch.Tensor, hist) -> None:
    """Write what run() returned for the timed window: the weight vector
    (float32, or float64 when the solve ran in float64) and the loss history
    (float64). A weight vector over the budget is written as a fixed, seeded
    sample, with the sampled indices alongside."""
    os.makedirs(out_dir, exist_ok=True)
    h = np.asarray(hist, dtype=np.float64)
    w = weights.detach().to("cpu")
    w = w.numpy().astype(np.float64 if w.dtype == torch.float64 else np.float32)
    budget = DUMP_BUDGET_BYTES - h.nbytes - 4096  # .npy headers
    if w.nbytes > budget:
        k = budget // (w.itemsize + 8)  # value + int64 index per sample
        idx = np.sort(np.random.RandomState(0).choice(w.size, size=k, replace=False))
        np.save(os.path.join(out_dir, "weights_sample_index.npy"), idx.astype(np.float64))
        w = w[idx]
    np.save(os.path.join(out_dir, "weights.npy"), w)
    np.save(os.path.join(out_dir, "loss_history.npy"), h)


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rows", type=int, default=16384, help="rows per GPU (weak scaling)")
    # --dim is an alias for --d: torchrun's own argparse abbreviation-matches
    # a bare --d before the script args when launching under
    # torch.distributed.run, so multi-rank launches must use --dim
    p.add_argument("--d", "--dim", dest="d", type=int, default=1_000_000)
    p.add_argument("--label-noise", type=float, default=0.1,
                   help="planted-model label noise; ~1.0 makes the problem "
                        "non-separable (persistent hinge-active rows)")
    p.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "f32", "f8"])
    p.add_argument("--loss", type=str, default="logistic", choices=list(LOSSES))
    # Default L2 reg 1e-3: with n << d any synthetic labeling is linearly
    # separable, so the unregularized logistic optimum is L* = 0 at infinity
    # and iters-to-eps is ill-defined. The small ridge makes the objective
    # strongly convex (well-defined, converged L*); throughput is measured
    # identical with/without it (profiles/bench_d1e6_l2.log vs bench_d1e6.log:
    # 10.14 vs 10.15 ms/step — the L2 prox is fused into the update kernel).
    p.add_argument("--reg", type=float, default=1e-3)
    p.add_argument("--csr", action="store_true", help="CSR-sparse shard instead of dense")
    p.add_argument("--nnz-per-row", type=int, default=64)
    p.add_argument("--csr-dist", type=str, default="uniform",
                   choices=["uniform", "zipf"],
                   help="column popularity: uniform, or zipf (power-law)")
    p.add_argument("--csr-zipf-a", type=float, default=1.1)
    p.add_argument("--csr-cluster", action="store_true",
                   help="column-frequency clustering preprocessing "
                        "(reindex_columns) before training")
    p.add_argument("--mixed", action="store_true",
                   help="heterogeneous shard: half the rows dense, half "
                        "CSR-sparse, over one feature space (MixedShard)")
    p.add_argument("--classes", type=int, default=0,
                   help=">0: multinomial softmax regression with K classes")
    p.add_argument("--eps", type=float, default=1e-3,
                   help="iters-to-eps tolerance: iterations to loss <= (1+eps)*L*")
    p.add_argument("--eps-iters", type=int, default=-1,
                   help="with --full: extra (untimed) iterations past the timed "
                        "window used to estimate L* for iters-to-eps; "
                        "-1 = auto, 0 = skip")
    p.add_argument("--full", action="store_true",
                   help="also run the untimed convergence run behind "
                        "iters-to-eps (off by default: a plain run only "
                        "times its steps)")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="write the timed run's outputs (weights, loss "
                        "history) as DIR/<name>.npy")
    p.add_argument("--streamed", action="store_true",
                   help="features in pinned host memory, double-buffered H2D "
                        "streaming (PCIe-bound capacity mode)")
    p.add_argument("--solver", type=str, default="direct", choices=["direct", "gram"],
                   help="gram = dual-space solver (K=A.A^T precompute; O(n_local*n_global) iterations)")
    args = p.parse_args()

    comm = init_from_env()
    rank, world = comm.rank, comm.world_size
    if args.gpus != world and rank == 0:
        print(f"[bench] note: --gpus {args.gpus} but WORLD_SIZE={world}; "
              "the record reports the ACTUAL world size", file=sys.stderr)
    if torch.cuda.is_available():
        device = torch.device("cuda", torch.cuda.current_device())
        dtype = {"bf16": torch.bfloat16, "f32": torch.float32,
                 "f8": torch.float8_e4m3fn}[args.dtype]
        wdtype = torch.float32
    else:  # CPU smoke fallback (the real bench runs on MI355X)
        device = torch.device("cpu")
        dtype = torch.float32
        wdtype = torch.float64
        args.rows = min(args.rows, 2048)
        args.d = min(args.d, 512)

    loss_type, grad_cls = LOSSES[args.loss]

    t_gen0 = time.perf_counter()
    if args.mixed and (args.classes > 0 or args.csr):
        raise SystemExit("--mixed is a binary dense+CSR configuration")
    if args.classes > 0 and args.csr:
        from sparkagd_amd.data import generate_multiclass_csr_problem

        shard, _w_true = generate_multiclass_csr_problem(
            args.rows, args.d, args.nnz_per_row, args.classes,
            seed=1234 + rank * 7, device=device,
        )
    elif args.classes > 0:
        from sparkagd_amd.data import generate_multiclass_problem

        shard, _w_true = generate_multiclass_problem(
            args.rows, args.d, args.classes, seed=1234 + rank * 7,
            device=device, dtype=dtype if device.type == "cuda" else torch.float64,
        )
    elif args.csr:
        shard, _w_true = generate_csr_problem(
            args.rows, args.d, args.nnz_per_row, seed=1234 + rank * 7,
            loss_type=loss_type, device=device, col_dist=args.csr_dist,
            zipf_a=args.csr_zipf_a,
        )
        if args.csr_cluster:
            from sparkagd_amd.data import reindex_columns

            shard, _perm = reindex_columns(shard)
    elif args.mixed:
        from sparkagd_amd.data import MixedShard

        half = max(args.rows // 2, 1)
        dense_part, _w_true = generate_dense_problem(
            half, args.d, seed=1234 + rank * 7, loss_type=loss_type,
            device=device, dtype=dtype, label_noise=args.label_noise,
        )
        csr_part, _ = generate_csr_problem(
            args.rows - half, args.d, args.nnz_per_row,
            seed=4321 + rank * 7, loss_type=loss_type, device=device,
            col_dist=args.csr_dist, zipf_a=args.csr_zipf_a,
        )
        shard = MixedShard([dense_part, csr_part])
    else:
        shard, _w_true = generate_dense_problem(
            args.rows, args.d, seed=1234 + rank * 7, loss_type=loss_type,
            device=device, dtype=dtype, label_noise=args.label_noise,
        )
    if args.solver == "gram" and args.csr:
        raise SystemExit("--solver gram needs a dense shard (K = A·Aᵀ is "
                         "dense n×n and the CSR configs have n ≥ 1e6 — "
                         "see sparkagd_amd/gram.py)")
    if args.streamed:
        if args.classes > 0 or args.csr or args.mixed:
            raise SystemExit("--streamed supports the dense binary configs")
        from sparkagd_amd import HostStreamedDenseShard

        shard = HostStreamedDenseShard(
            shard.features.cpu(), shard.labels,
            device=device, chunk_rows=min(args.rows, 1024))
    sync(device)
    t_gen = time.perf_counter() - t_gen0

    if args.classes > 0:
        gradient = CountingGradient(MultinomialLogisticGradient(args.classes))
        w0 = torch.zeros(args.d * args.classes, device=device,
                         dtype=torch.float32 if device.type == "cuda" else torch.float64)
    else:
        gradient = CountingGradient(grad_cls())
        w0 = torch.zeros(args.d, device=device, dtype=wdtype)
    updater = SquaredL2Updater() if args.reg > 0 else SimpleUpdater()

    gram_op = None
    gram_build_seconds = None
    if args.solver == "gram":
        # build K OUTSIDE the timed region (like data generation) and
        # disclose the cost in the config block
        from sparkagd_amd import GramOperator

        gram_op = GramOperator(shard, comm)
        sync(device)
        gram_build_seconds = round(gram_op.build_seconds, 3)

    state = {"t0": 0.0, "t1": 0.0, "e0": 0, "e1": 0, "p0": 0, "p1": 0, "timed_iters": 0}
    total_iters = args.warmup + args.steps
    # Convergence run AFTER the timed one (--full only): an untimed run past
    # the timed window's length that drives the trajectory near its optimum
    # so L* (= min over the whole history) is converged and iters-to-eps is
    # well-defined. Auto: enough to converge the bench configs, capped so it
    # stays a few seconds.
    eps_iters = args.eps_iters if args.full else 0
    if eps_iters < 0:
        # 300 total on GPU: converges every bench config for a stable L*
        eps_iters = 300 if device.type == "cuda" else 60
        eps_iters = max(0, eps_iters - total_iters)  # long runs converge alone

    def hook(n_iter: int):
        if n_iter == args.warmup:
            comm.barrier()
            sync(device)
            state["t0"] = time.perf_counter()
            state["e0"] = gradient.n_evals
            state["p0"] = gradient.n_passes
        if n_iter == total_iters:
            comm.barrier()
            sync(device)
            state["t1"] = time.perf_counter()
            state["e1"] = gradient.n_evals
            state["p1"] = gradient.n_passes
            state["timed_iters"] = n_iter - args.warmup
            return "stop"
        return None

    if args.warmup == 0:
        comm.barrier()
        sync(device)
        state["t0"] = time.perf_counter()

    weights, hist = run(
        shard, gradient, updater,
        0.0,                      # convergence_tol: never stop early in a bench
        total_iters, args.reg, w0,
        1.0, math.inf, 0.5, 0.9, True,
        loss_history_mode="backtrack",
        comm=comm,
        iteration_hook=hook,
        solver=args.solver,
        gram_op=gram_op,
    )

    if state["t1"] == 0.0:  # early break (e.g. exact convergence): close the
        comm.barrier()      # timing window at the actual stop point
        sync(device)
        state["t1"] = time.perf_counter()
        state["e1"] = gradient.n_evals
        state["p1"] = gradient.n_passes
        state["timed_iters"] = max(len(hist) - args.warmup, 1)

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, weights, hist)

    if eps_iters > 0:
        # the same trajectory from w0 (seeded inputs, replicated control
        # flow), carried eps_iters past the timed window; its history
        # replaces the timed run's for L*, iters-to-eps and loss_final
        _w_tail, hist = run(
            shard, gradient, updater,
            0.0, total_iters + eps_iters, args.reg, w0,
            1.0, math.inf, 0.5, 0.9, True,
            loss_history_mode="backtrack",
            comm=comm,
            solver=args.solver,
            gram_op=gram_op,
        )

    elapsed_local = state["t1"] - state["t0"]
    evals = state["e1"] - state["e0"]
    passes = state["p1"] - state["p0"]
    timed_iters = state["timed_iters"] or args.steps

    # elapsed = MAX over ranks
    el = torch.tensor([elapsed_local], dtype=torch.float64, device=device)
    if world > 1:
        import torch.distributed as dist

        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    elapsed = float(el[0])

    global_rows = args.rows * world
    # value counts EVALUATION-examples (rows x loss evaluations; each AGD
    # step makes 2 evaluations); rows_per_sec is the same window counted in
    # rows x steps — both emitted so the headline cannot be misread.
    examples = global_rows * evals  # evals identical on all ranks (replicated control flow)
    value = examples / elapsed if elapsed > 0 else float("nan")
    rows_per_sec = global_rows * timed_iters / elapsed if elapsed > 0 else float("nan")

    # vs_baseline: BASELINE.md's measured round-1 headline (3.23M
    # eval-examples/s on 1 MI355X, dense logistic d=1e6 bf16 16384 rows/GPU);
    # under weak scaling the N-GPU baseline is N x the 1-GPU number.
    vs_baseline = None
    if (device.type == "cuda" and not args.csr and args.classes == 0
            and not args.streamed and args.loss == "logistic"
            and args.d == 1_000_000 and args.rows == 16384
            and args.solver == "direct" and args.dtype == "bf16"):
        vs_baseline = value / (3.23e6 * world)

    # iters-to-eps: first iteration with loss <= (1+eps)*L*, L* = min over
    # the convergence run's history (--full) — the single definition
    # shared with benchmarks/iters_to_eps.py (utils.metrics.iters_to_eps).
    iters_to_eps = _iters_to_eps(hist, args.eps) if eps_iters > 0 or len(hist) >= 60 else None

    if rank == 0:
        out = {
            "metric": BASELINE_METRIC,
            "value": value,
            "unit": "examples/s",
            "n_gpus": world,
            "steps": timed_iters,
            "warmup": args.warmup,
            "ms_per_step": elapsed * 1000.0 / timed_iters,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": vs_baseline,
            "dtype": (("f32" if args.csr else (f"{args.dtype}+f32" if args.mixed else args.dtype)) if device.type == "cuda" else "f32"),
            "data": "synthetic",
            "rows_per_sec": rows_per_sec,
            "config": {
                "model": (f"{'csr_' if args.csr else ''}multinomial{args.classes}_regression"
                          if args.classes > 0
                          else f"{'csr' if args.csr else ('streamed' if args.streamed else ('mixed' if args.mixed else 'dense'))}_{args.loss}_regression"),
                "d": args.d,
                "rows_per_gpu": args.rows,
                "global_rows": global_rows,
                "parallelism": f"dp{world}",
                "solver": args.solver,
                "reg_param": args.reg,
                "label_noise": args.label_noise,
                "csr_dist": args.csr_dist if (args.csr or args.mixed) else None,
                "csr_cluster": bool(args.csr_cluster) if args.csr else None,
                "evals_per_step": evals / max(timed_iters, 1),
                "data_passes_per_step": passes / max(timed_iters, 1),
                "examples_definition": "rows x loss_evaluations (2 evals/AGD step); rows_per_sec = rows x steps / s",
                "weights_dtype": str(wdtype).replace("torch.", ""),
                "loss_final": hist[-1] if hist else None,
                "iters_to_eps": iters_to_eps,
                "eps": args.eps,
                "eps_iters_tail": eps_iters,
                "loss_star": min(hist) if hist else None,
                "gen_seconds": round(t_gen, 3),
                "gram_build_seconds": gram_build_seconds,
                "shard_gb": round(shard.nbytes / 2**30, 3),
            },
        }
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
