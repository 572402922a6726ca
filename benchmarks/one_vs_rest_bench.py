#!/usr/bin/env python3
"""One-vs-rest multiclass training as ONE stacked run against K sequential
binary runs, on one MI355X.

One bf16 dense shard (262144 x 10240 by default) with K = 16 classes,
logistic loss, squared-L2 regulariser, timed two ways:

    stacked      the run OneVsRestWithAGD.train makes: MultiTaskGradient with
                 a target class per column over the [d, K] weight block, one
                 lambda, margins tracked (two shard streams per step)
    sequential   K single-model runs of LogisticGradient (what
                 LogisticRegressionWithAGD.train makes) on the same features
                 with the labels relabelled [label == c]; the figure is the
                 SUM of the K runs' ms/step

Each timed unit is one run() of --warmup + --steps iterations whose last
--steps are bracketed by device synchronises. The two ways alternate, one of
each per round, after one untimed round; the figures are the median, minimum
and maximum over --rounds rounds.

Then the n-space kernel alone: k_multiplier_tasks_ovr<16> against
k_multiplier_tasks<16> on the same [n, 16] margins (the binary kernel sees
the labels relabelled for class 0), timed with device events over --reps
calls after --reps untimed ones, alternating, --rounds rounds.

--intercept instead compares the stacked run with and without a bias per
class (MultiTaskGradient(intercept=True) with PerTaskUpdater(free_rows=1), the
run OneVsRestWithAGD.train(intercept=True) makes) under the same alternating
protocol, then times the three n-space bias kernels per call with device
events: k_colsum_multi, k_add_bias_cols and k_at_margin_update_tasks_off
(next to k_at_margin_update_tasks, which it replaces).
Needs a GPU: there is no CPU fallback for a timing.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.cv_sweep_bench import DEV, timed_run  # noqa: E402
from sparkagd_amd import (DenseShard, LogisticGradient,  # noqa: E402
                          MultiTaskGradient, PerTaskUpdater,
                          SquaredL2Updater, ops)
from sparkagd_amd.data import generate_multiclass_problem  # noqa: E402
from sparkagd_amd.ops import multitask as mt  # noqa: E402
from sparkagd_amd.ops.multiclass import padded_k  # noqa: E402


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs),
            "rounds": xs}


def event_ms(fn, reps):
    """ms per call over ``reps`` calls between two device events, after
    ``reps`` untimed calls."""
    for _ in range(reps):
        fn()
    start, stop = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def intercept_rounds(args, shard, k, out):
    """Stacked run without / with intercepts, alternating, then the three
    n-space bias kernels alone."""
    l2 = SquaredL2Updater()
    plain = MultiTaskGradient(LogisticGradient(), k, target_class=range(k))
    biased = MultiTaskGradient(LogisticGradient(), k, target_class=range(k),
                               intercept=True)
    free = PerTaskUpdater(l2, [args.lam] * k, free_rows=1)

    def without():
        return timed_run(shard, plain, l2, args.lam, shard.d * k, args.warmup,
                         args.steps, True)

    def with_bias():
        return timed_run(shard, biased, free, 1.0, (shard.d + 1) * k,
                         args.warmup, args.steps, True)

    def per_task():
        # no bias, but the kernel sequence of the intercept run (per-column
        # margin update, no fused step tail): isolates what the bias adds
        return timed_run(shard, plain, PerTaskUpdater(l2, [args.lam] * k),
                         1.0, shard.d * k, args.warmup, args.steps, True)

    without(), with_bias(), per_task()  # untimed: code objects, allocator
    a, b, c = [], [], []
    for _ in range(args.rounds):
        a.append(without())
        b.append(with_bias())
        c.append(per_task())
    out["stacked_ms_per_step"], out["stacked_intercept_ms_per_step"] = spread(a), spread(b)
    out["stacked_per_task_updater_ms_per_step"] = spread(c)
    for name, r in (("stacked (plain updater)  ", out["stacked_ms_per_step"]),
                    ("stacked + intercepts     ", out["stacked_intercept_ms_per_step"]),
                    ("stacked, per-task updater", out["stacked_per_task_updater_ms_per_step"])):
        print(f"  {name} median {r['median']:9.3f} ms/step  min {r['min']:9.3f}"
              f"  max {r['max']:9.3f}", flush=True)
    diff = statistics.median(b) - statistics.median(a)
    width = max(max(a) - min(a), max(b) - min(b))
    print(f"  intercepts cost {diff:+.3f} ms/step (medians); the larger of the "
          f"two spreads (max - min) is {width:.3f} ms", flush=True)
    print(f"  against the per-task updater's sequence without a bias: "
          f"{statistics.median(b) - statistics.median(c):+.3f} ms/step",
          flush=True)

    kc = padded_k(k)
    n = args.rows
    zm, xm, gm = (torch.randn(n * kc, device=DEV) for _ in range(3))
    w = torch.randn((shard.d + 1) * k, device=DEV)
    lam = torch.full((k,), args.lam, dtype=torch.float64, device=DEV)
    tail = torch.empty(k, device=DEV)
    kernels = {
        "colsum_multi": lambda: mt.colsum_multi(zm, k, tail=tail, want_f64=False),
        "add_bias_cols": lambda: mt.add_bias_cols(zm, 1.0, w, shard.d * k, k),
        "at_margin_update_tasks_off": lambda: mt.at_margin_update_tasks(
            zm, xm, gm, 0.5, lam, 0.5, k, offset=(w, shard.d * k)),
        "at_margin_update_tasks": lambda: mt.at_margin_update_tasks(
            zm, xm, gm, 0.5, lam, 0.5, k),
    }
    times = {name: [] for name in kernels}
    for _ in range(args.rounds):
        for name, fn in kernels.items():
            times[name].append(event_ms(fn, args.reps))
    out["bias_kernels_ms"] = {name: spread(v) for name, v in times.items()}
    for name, r in out["bias_kernels_ms"].items():
        print(f"  {name:28s} median {r['median']:7.4f} ms/call  min "
              f"{r['min']:7.4f}  max {r['max']:7.4f}", flush=True)
    print(f"  [n, KC] = [{n}, {kc}] f32: {n * kc * 4 / 1e6:.1f} MB per flat",
          flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=262144)
    p.add_argument("--d", type=int, default=10240)
    p.add_argument("--classes", type=int, default=16)
    p.add_argument("--lam", type=float, default=1e-3)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--intercept", action="store_true",
                   help="stacked run with against without a bias per class, "
                        "and the n-space bias kernels alone")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("one_vs_rest_bench needs a GPU (no CPU fallback for timings)")
    torch.cuda.set_device(0)
    k = args.classes
    shard, _ = generate_multiclass_problem(args.rows, args.d, k, seed=0,
                                           device=DEV, dtype=torch.bfloat16)
    print(f"dense bf16 {args.rows} x {args.d} ({shard.nbytes / 1e9:.1f} GB), "
          f"K = {k}, lambda {args.lam:g}, {args.warmup} + {args.steps} steps, "
          f"{args.rounds} rounds", flush=True)
    if args.intercept:
        out = {"rows": args.rows, "d": args.d, "classes": k, "lam": args.lam,
               "warmup": args.warmup, "steps": args.steps,
               "rounds": args.rounds, "reps": args.reps,
               "shard_packed_by_policy": bool(shard.is_packed)}
        intercept_rounds(args, shard, k, out)
        print("RESULT " + json.dumps(out), flush=True)
        return
    l2 = SquaredL2Updater()
    ovr = MultiTaskGradient(LogisticGradient(), k, target_class=range(k))
    binary = DenseShard(shard.features, shard.labels)

    def stacked():
        return timed_run(shard, ovr, l2, args.lam, shard.d * k, args.warmup,
                         args.steps, True)

    def sequential():
        total = 0.0
        for c in range(k):
            binary.labels = (shard.labels == c).to(torch.float32)
            total += timed_run(binary, LogisticGradient(), l2, args.lam,
                               shard.d, args.warmup, args.steps)
        return total

    stacked(), sequential()  # one untimed round: code objects, allocator
    s, q = [], []
    for _ in range(args.rounds):
        s.append(stacked())
        q.append(sequential())
    out = {"rows": args.rows, "d": args.d, "classes": k, "lam": args.lam,
           "warmup": args.warmup, "steps": args.steps, "rounds": args.rounds,
           "stacked_ms_per_step": spread(s),
           "sequential_sum_ms_per_step": spread(q),
           "shards_packed_by_policy": [bool(shard.is_packed),
                                       bool(binary.is_packed)]}
    for name, r in (("stacked   ", out["stacked_ms_per_step"]),
                    ("sequential", out["sequential_sum_ms_per_step"])):
        print(f"  {name} median {r['median']:9.3f} ms/step  min {r['min']:9.3f}"
              f"  max {r['max']:9.3f}", flush=True)
    print(f"  stacked is {statistics.median(q) / statistics.median(s):.2f}x "
          f"faster than the {k} sequential runs", flush=True)

    # the n-space kernel alone
    kc = padded_k(k)
    z = torch.randn(args.rows * kc, device=DEV)
    scale = torch.ones(k, device=DEV)
    target = torch.arange(k, dtype=torch.int32, device=DEV)
    y0 = (shard.labels == 0).to(torch.float32)
    a, b = [], []
    for _ in range(args.rounds):
        a.append(event_ms(lambda: mt.multiplier_tasks(
            z, shard.labels, ops.LOSS_LOGISTIC, k, scale, target=target), args.reps))
        b.append(event_ms(lambda: mt.multiplier_tasks(
            z, y0, ops.LOSS_LOGISTIC, k, scale), args.reps))
    out["multiplier_ovr_ms"], out["multiplier_binary_ms"] = spread(a), spread(b)
    for name, r in (("k_multiplier_tasks_ovr<16>", out["multiplier_ovr_ms"]),
                    ("k_multiplier_tasks<16>    ", out["multiplier_binary_ms"])):
        print(f"  {name} median {r['median']:7.4f} ms/call  min {r['min']:7.4f}"
              f"  max {r['max']:7.4f}   (call = kernel + finish + allocations)",
              flush=True)
    print(f"  one-vs-rest / binary: "
          f"{statistics.median(a) / statistics.median(b):.3f}", flush=True)
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
