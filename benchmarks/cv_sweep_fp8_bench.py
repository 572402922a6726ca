#!/usr/bin/env python3
"""The batched CV sweep of cv_sweep_bench.py on an fp8 shard, on one MI355X.

One set of values (262144 x 10240 by default) held twice, as a bf16 shard
and as its float8_e4m3fn rounding; logistic loss, mixed lambdas through
PerTaskUpdater, margins tracked, R = 5 lambdas x 3 folds = 15 columns
(KC = 16). One batched run() per way:

    bf16_gemm   the bf16 shard on the hipBLASLt NT / TN GEMMs (2 B/element)
    fp8_valu    the fp8 shard on k_margins_multi<u8> / k_grad_multi<u8>: the
                default up to 32 padded columns
    fp8_mfma    the fp8 shard on k_margins_multi_f8 / k_grad_multi_f8, chosen
                by SPARKAGD_MULTI_MARGINS=mfma and SPARKAGD_MULTI_GRAD=mfma

The ways alternate, one of each per round, after one untimed round; the
figures are the median and minimum ms/step over --rounds rounds (timed_run
of cv_sweep_bench.py). --ops adds the two data passes alone, timed with
device events over --steps calls after one warm call each, as TB/s of shard
bytes. --ways restricts the run (a kernel trace wants fp8_mfma alone).
Needs a GPU: there is no CPU fallback for a timing.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cv_sweep_bench import DEV, timed_run  # noqa: E402
from sparkagd_amd import (DenseShard, LogisticGradient,  # noqa: E402
                          MultiTaskGradient, PerTaskUpdater, SquaredL2Updater,
                          assign_folds, ops)
from sparkagd_amd.data import generate_dense_problem  # noqa: E402
from sparkagd_amd.ops import multiclass as mc  # noqa: E402

WAYS = ("bf16_gemm", "fp8_valu", "fp8_mfma")
ENV = ("SPARKAGD_MULTI_MARGINS", "SPARKAGD_MULTI_GRAD")


def select(way):
    """Point the two routing variables at ``way``'s kernels."""
    for name in ENV:
        os.environ.pop(name, None)
        if way == "fp8_mfma":
            os.environ[name] = "mfma"


def event_ms(fn, steps):
    fn()  # code objects, allocator
    t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


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
    p.add_argument("--ways", nargs="+", choices=WAYS, default=list(WAYS))
    p.add_argument("--ops", action="store_true",
                   help="also time the margins and gradient passes alone")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cv_sweep_fp8_bench needs a GPU (no CPU fallback for timings)")
    torch.cuda.set_device(0)
    bf16, _ = generate_dense_problem(args.rows, args.d, seed=0, device=DEV,
                                     dtype=torch.bfloat16)
    fp8 = DenseShard(bf16.features.to(torch.float8_e4m3fn), bf16.labels)
    shards = {"bf16_gemm": bf16, "fp8_valu": fp8, "fp8_mfma": fp8}
    folds = assign_folds(args.rows, args.folds, seed=0)
    holdout = [f for _ in args.lambdas for f in range(args.folds)]
    task_lams = [lam for lam in args.lambdas for _ in range(args.folds)]
    r = len(holdout)
    grad = MultiTaskGradient(LogisticGradient(), r, folds, holdout)
    upd = PerTaskUpdater(SquaredL2Updater(), task_lams)
    print(f"dense {args.rows} x {args.d}: bf16 {bf16.nbytes / 1e9:.2f} GB, fp8 "
          f"{fp8.nbytes / 1e9:.2f} GB; {r} tasks (KC = {mc.padded_k(r)}), "
          f"{args.warmup} + {args.steps} steps, {args.rounds} rounds", flush=True)

    def batched(way):
        select(way)
        return timed_run(shards[way], grad, upd, 1.0, args.d * r, args.warmup,
                         args.steps, True)

    out = {"rows": args.rows, "d": args.d, "tasks": r, "steps": args.steps,
           "rounds": args.rounds}
    for way in args.ways:  # one untimed round
        batched(way)
    times = {way: [] for way in args.ways}
    for _ in range(args.rounds):
        for way in args.ways:
            times[way].append(batched(way))
    for way in args.ways:
        t = times[way]
        out[way] = {"ms_per_step": statistics.median(t), "min": min(t), "rounds": t}
        print(f"  {way:10s} median {statistics.median(t):9.3f} ms/step  min "
              f"{min(t):9.3f}  max {max(t):9.3f}", flush=True)

    if args.ops:
        kc = mc.padded_k(r)
        g = torch.Generator(device=DEV).manual_seed(1)
        w = 0.01 * torch.randn(args.d * r, device=DEV, generator=g)
        m = torch.zeros(args.rows, kc, device=DEV)
        m[:, :r] = torch.randn(args.rows, r, device=DEV, generator=g)
        m = m.reshape(-1)
        out["ops"] = {}
        for way in args.ways:
            select(way)
            feats = shards[way].features
            passes = {
                "margins": lambda: mc.margins_multi(feats, w, r),
                "gradient": lambda: mc.grad_from_mult_multi(feats, m, r),
            }
            if way == "fp8_mfma":  # M rounded to bf16 once, as the TN GEMM does
                passes["gradient_bf16_m"] = lambda: ops.grad_multi_fp8(feats, m, r)
            for name, fn in passes.items():
                ms = event_ms(fn, args.steps)
                tbs = feats.numel() * feats.element_size() / (ms * 1e-3) / 1e12
                out["ops"][f"{way}.{name}"] = {"ms": ms, "shard_tb_per_s": tbs}
                print(f"  {way:10s} {name:16s} {ms:8.3f} ms  {tbs:5.2f} TB/s of "
                      "shard bytes", flush=True)
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
