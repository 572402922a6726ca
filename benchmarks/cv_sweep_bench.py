#!/usr/bin/env python3
"""A cross-validation sweep as ONE batched run against R sequential runs, on
one MI355X.

One bf16 dense shard (262144 x 10240 by default), logistic loss, squared-L2
regulariser, R = 15 tasks from 5 lambdas x 3 folds, timed three ways:

    batched      one run() of MultiTaskGradient over the [d, R] weight block:
                 every stream of the shard serves all R tasks; margins
                 tracked (two shard streams per step; track_margins=True,
                 which a mixed sweep on a bf16 GPU shard needs to opt in)
    untracked    the same batched run with track_margins=False (three
                 streams per step) — mixed-lambda sweep only
    sequential   R single-task run() calls, one per (lambda, fold), each on
                 the WHOLE shard — not on the 2/3 of its rows a fold's
                 training set holds — so the figure is also reported scaled
                 by 2/3, the fair lower bound for a sequential sweep

and under two sweeps: every lambda equal (plain SquaredL2Updater, the scalar
fused margin update) and mixed lambdas (PerTaskUpdater, the per-column margin
update k_at_margin_update_tasks). The untracked way is the mixed sweep before
that kernel existed and what an L1 or elastic-net sweep still runs: the A/B
of tracking comes from one alternating run.

Each timed unit is one run() of --warmup + --steps iterations whose last
--steps are bracketed by device synchronises; the sequential figure is the
SUM of the R runs' ms/step. The ways alternate, one of each per round, after
one untimed round; the figures are the median and minimum over --rounds
rounds. Needs a GPU: there is no CPU fallback for a timing.
"""

import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sparkagd_amd import (LogisticGradient, MultiTaskGradient,  # noqa: E402
                          PerTaskUpdater, SquaredL2Updater, assign_folds, run)
from sparkagd_amd.data import generate_dense_problem  # noqa: E402

DEV = "cuda:0"


def timed_run(shard, gradient, updater, reg, dim, warmup, steps,
              track_margins="auto"):
    """ms per step over the last ``steps`` of one run of warmup + steps
    iterations from zero weights."""
    w0 = torch.zeros(dim, device=DEV, dtype=torch.float32)
    t = {}

    def hook(n_iter):
        if n_iter == warmup:
            torch.cuda.synchronize()
            t["t0"] = time.perf_counter()
        if n_iter == warmup + steps:
            torch.cuda.synchronize()
            t["t1"] = time.perf_counter()
            return "stop"
        return None

    _w, hist = run(shard, gradient, updater, 0.0, warmup + steps, reg, w0,
                   1.0, math.inf, 0.5, 0.9, True,
                   loss_history_mode="backtrack", iteration_hook=hook,
                   track_margins=track_margins)
    if "t1" not in t or len(hist) != warmup + steps:
        raise RuntimeError("run stopped before the timed window closed")
    return (t["t1"] - t["t0"]) * 1e3 / steps


def sweep(shard, folds, n_folds, lams, warmup, steps, rounds):
    holdout = [f for _ in lams for f in range(n_folds)]
    task_lams = [lam for lam in lams for _ in range(n_folds)]
    r = len(holdout)
    grad = MultiTaskGradient(LogisticGradient(), r, folds, holdout)
    l2 = SquaredL2Updater()
    mixed = len(set(task_lams)) > 1
    if mixed:
        upd, reg = PerTaskUpdater(l2, task_lams), 1.0
    else:
        upd, reg = l2, task_lams[0]

    def batched(track_margins=True):
        return timed_run(shard, grad, upd, reg, shard.d * r, warmup, steps,
                         track_margins)

    def sequential():
        return sum(timed_run(shard, LogisticGradient(), l2, lam, shard.d,
                             warmup, steps) for lam in task_lams)

    # one untimed round: code objects, allocator
    batched(), (batched(False) if mixed else None), sequential()
    b, u, s = [], [], []
    for _ in range(rounds):
        b.append(batched())
        if mixed:
            u.append(batched(False))
        s.append(sequential())
    res = {}
    if mixed:
        res = {"untracked_ms_per_step": statistics.median(u),
               "untracked_min": min(u), "untracked_rounds": u}
    return {**res, "tasks": r,
            "batched_ms_per_step": statistics.median(b),
            "batched_min": min(b),
            "batched_rounds": b,
            "sequential_sum_ms_per_step": statistics.median(s),
            "sequential_min": min(s),
            "sequential_two_thirds": statistics.median(s) * 2.0 / 3.0}


def report(title, res):
    b, s, s23 = (res["batched_ms_per_step"], res["sequential_sum_ms_per_step"],
                 res["sequential_two_thirds"])
    print(title, flush=True)
    print(f"  batched     median {b:9.3f} ms/step  min {res['batched_min']:9.3f}"
          f"   ({res['tasks']} tasks in one run, margins tracked)", flush=True)
    if "untracked_ms_per_step" in res:
        u = res["untracked_ms_per_step"]
        print(f"  untracked   median {u:9.3f} ms/step  min {res['untracked_min']:9.3f}"
              f"   (the same run, track_margins=False: {u / b:.2f}x the tracked)",
              flush=True)
    print(f"  sequential  median {s:9.3f} ms/step  min {res['sequential_min']:9.3f}"
          f"   (sum of {res['tasks']} runs, each on the WHOLE shard)", flush=True)
    print(f"  sequential x 2/3   {s23:9.3f} ms/step"
          "   (fair lower bound: a fold trains on 2/3 of the rows)", flush=True)
    print(f"  batched is {s / b:.2f}x faster than sequential, "
          f"{s23 / b:.2f}x against the 2/3-scaled figure", flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=262144)
    p.add_argument("--d", type=int, default=10240)
    p.add_argument("--folds", type=int, default=3)
    p.add_argument("--lambdas", type=float, nargs="+",
                   default=[1e-5, 1e-4, 1e-3, 1e-2, 1e-1])
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--rounds", type=int, default=5)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cv_sweep_bench needs a GPU (no CPU fallback for timings)")
    torch.cuda.set_device(0)
    shard, _ = generate_dense_problem(args.rows, args.d, seed=0, device=DEV,
                                      dtype=torch.bfloat16)
    folds = assign_folds(args.rows, args.folds, seed=0)
    print(f"dense bf16 {args.rows} x {args.d} ({shard.nbytes / 1e9:.1f} GB), "
          f"{len(args.lambdas)} lambdas x {args.folds} folds, "
          f"{args.warmup} + {args.steps} steps, {args.rounds} rounds", flush=True)
    print("NOTE: the sequential runs use the whole shard, not the 2/3 of its "
          "rows a fold trains on; 'sequential x 2/3' is the fair lower bound.",
          flush=True)
    out = {"rows": args.rows, "d": args.d, "folds": args.folds,
           "lambdas": args.lambdas, "warmup": args.warmup,
           "steps": args.steps, "rounds": args.rounds}
    mid = args.lambdas[len(args.lambdas) // 2]
    out["equal_lambda_tracked"] = sweep(
        shard, folds, args.folds, [mid] * len(args.lambdas), args.warmup,
        args.steps, args.rounds)
    report(f"equal lambda ({mid:g}): plain updater, margins tracked",
           out["equal_lambda_tracked"])
    out["mixed_lambda"] = sweep(
        shard, folds, args.folds, args.lambdas, args.warmup, args.steps,
        args.rounds)
    report("mixed lambdas: PerTaskUpdater, margins tracked per column",
           out["mixed_lambda"])
    out["shard_packed_by_policy"] = bool(shard.is_packed)
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
