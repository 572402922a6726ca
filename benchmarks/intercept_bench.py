#!/usr/bin/env python3
"""AGD step time with and without an intercept, on one MI355X.

One bf16 dense shape (the flagship 16384 x 1e6 by default) and one CSR
shape, logistic loss, SquaredL2Updater, timed three ways:

    plain        no intercept: the shard as it is, weights [d]
    intercept    InterceptShard + FreeTailUpdater: weights [d + 1], the
                 feature stream untouched, the bias in n-length kernels
    ones column  data.add_intercept: an n x (d + 1) copy of the features
                 (dense only); d + 1 is odd, so the margins and gradient
                 kernels leave their 16-byte lane loads for the scalar path,
                 and the regulariser sees the bias

Each timed unit is one run() of --warmup + --steps iterations whose last
--steps are bracketed by device synchronises (the bench.py bracket); the ways
are run in alternation, one of each per round, after one untimed round, and
the figures are the median and minimum ms/step over --rounds rounds, with the
evaluations per step each way needed (the trajectories differ, so the
backtracking may). ``plain`` on the same build is the yardstick for
``intercept``. ``--trace-way NAME`` runs only that way once, for a kernel
trace taken in a run of its own. Needs a GPU: there is no CPU fallback for a
timing.
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

from sparkagd_amd import (FreeTailUpdater, InterceptShard, LogisticGradient,  # noqa: E402
                          SquaredL2Updater, run)
from sparkagd_amd.data import (add_intercept, generate_csr_problem,  # noqa: E402
                               generate_dense_problem)

DEV = "cuda:0"


class _Evals:
    def __init__(self):
        self.n = []

    def log(self, **kw):
        self.n.append(kw["n_evals"])


def agd_steps(shard, updater, reg, warmup, steps):
    """(ms per step, evaluations per step) over the last ``steps`` of one
    run of warmup + steps iterations from zero weights."""
    w0 = torch.zeros(shard.d, device=DEV, dtype=torch.float32)
    t = {}
    rec = _Evals()

    def hook(n_iter):
        if n_iter == warmup:
            torch.cuda.synchronize()
            t["t0"] = time.perf_counter()
        if n_iter == warmup + steps:
            torch.cuda.synchronize()
            t["t1"] = time.perf_counter()
            return "stop"
        return None

    _w, hist = run(shard, LogisticGradient(), updater, 0.0, warmup + steps,
                   reg, w0, 1.0, math.inf, 0.5, 0.9, True,
                   loss_history_mode="backtrack", iteration_hook=hook,
                   metrics=rec)
    if "t1" not in t or len(hist) != warmup + steps:
        raise RuntimeError("run stopped before the timed window closed")
    return ((t["t1"] - t["t0"]) * 1e3 / steps,
            sum(rec.n[warmup:]) / steps)


def alternate(ways, reg, warmup, steps, rounds):
    for fn in ways.values():  # one untimed round: code objects, allocator
        fn(reg, warmup, steps)
    ms = {k: [] for k in ways}
    ev = {}
    for _ in range(rounds):
        for name, fn in ways.items():
            m, e = fn(reg, warmup, steps)
            ms[name].append(m)
            ev[name] = e
    return {k: {"median_ms_per_step": statistics.median(v),
                "min_ms_per_step": min(v), "evals_per_step": ev[k]}
            for k, v in ms.items()}


def report(title, res):
    print(title, flush=True)
    base = res["plain"]["median_ms_per_step"]
    for name, r in res.items():
        print(f"  {name:12s} median {r['median_ms_per_step']:9.3f} ms/step  "
              f"min {r['min_ms_per_step']:9.3f}  "
              f"{r['evals_per_step']:.2f} evals/step  "
              f"{r['median_ms_per_step'] / base:6.3f}x plain", flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=16384)
    p.add_argument("--d", type=int, default=1_000_000)
    p.add_argument("--csr-rows", type=int, default=1_000_000)
    p.add_argument("--csr-d", type=int, default=10_000_000)
    p.add_argument("--nnz-per-row", type=int, default=64)
    p.add_argument("--reg", type=float, default=1e-3)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--skip-copy", action="store_true",
                   help="leave out the ones-column copy (a second n x d allocation)")
    p.add_argument("--trace-way", default=None,
                   choices=["plain", "intercept", "ones column",
                            "csr plain", "csr intercept"],
                   help="run only this way once (for a kernel trace)")
    args = p.parse_args()
    if args.skip_copy and args.trace_way == "ones column":
        p.error("--trace-way 'ones column' needs the copy: drop --skip-copy")
    if not torch.cuda.is_available():
        raise SystemExit("intercept_bench needs a GPU (no CPU fallback for timings)")
    torch.cuda.set_device(0)
    l2 = SquaredL2Updater()
    tw = args.trace_way
    out = {"rows": args.rows, "d": args.d, "csr_rows": args.csr_rows,
           "csr_d": args.csr_d, "nnz_per_row": args.nnz_per_row,
           "reg": args.reg, "warmup": args.warmup, "steps": args.steps,
           "rounds": args.rounds}

    if tw is None or not tw.startswith("csr"):
        shard, _ = generate_dense_problem(args.rows, args.d, seed=0, device=DEV,
                                          dtype=torch.bfloat16)
        ways = {
            "plain": lambda *a: agd_steps(shard, l2, *a),
            "intercept": lambda *a: agd_steps(InterceptShard(shard),
                                              FreeTailUpdater(l2), *a),
        }
        if not args.skip_copy and tw in (None, "ones column"):
            copied = add_intercept(shard)
            ways["ones column"] = lambda *a: agd_steps(copied, l2, *a)
        if tw is not None:
            print(tw, ways[tw](args.reg, args.warmup, args.steps), flush=True)
            return
        out["dense"] = alternate(ways, args.reg, args.warmup, args.steps,
                                 args.rounds)
        report(f"dense bf16 {args.rows} x {args.d} "
               f"({shard.nbytes / 1e9:.1f} GB)", out["dense"])
        del shard, ways
        if not args.skip_copy:
            del copied
        torch.cuda.empty_cache()

    csr, _ = generate_csr_problem(args.csr_rows, args.csr_d, args.nnz_per_row,
                                  seed=0, device=DEV)
    ways = {
        "plain": lambda *a: agd_steps(csr, l2, *a),
        "intercept": lambda *a: agd_steps(InterceptShard(csr),
                                          FreeTailUpdater(l2), *a),
    }
    if tw is not None:
        print(tw, ways[tw[4:]](args.reg, args.warmup, args.steps), flush=True)
        return
    out["csr"] = alternate(ways, args.reg, args.warmup, args.steps, args.rounds)
    report(f"CSR {args.csr_rows} x {args.csr_d}, {args.nnz_per_row} nnz/row "
           f"({csr.nbytes / 1e9:.1f} GB, deterministic CSC gradient)",
           out["csr"])
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
