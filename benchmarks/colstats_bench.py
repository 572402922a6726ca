#!/usr/bin/env python3
"""Column statistics / feature scaling: measured cost on one MI355X, next to
the existing kernels that stream the same bytes once.

Dense (headline bf16 shard, 16384 x 1e6 = 32.8 GB):
    column_stats            vs  ops.dense_grad_from_mult (the A^T.m pass)
    StandardScaler.transform(inplace=True)
CSR (bench shard, 1e6 rows x 1e7 columns x 64 nnz/row):
    column_stats            vs  the CSC gradient pass
    StandardScaler.transform(inplace=True)

Times are device-event times around whole calls (kernels + their small
allocations), median and min over --reps after --warmup calls. TB/s is the
bytes the algorithm must move (computed from the shapes below) over the
median time. Needs a GPU: there is no CPU fallback for a timing.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sparkagd_amd import StandardScaler, column_stats, ops  # noqa: E402
from sparkagd_amd.data import generate_csr_problem, generate_dense_problem  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms), min(ms)


def report(name, nbytes, med, lo, out):
    tbs = nbytes / (med * 1e-3) / 1e12
    print(f"{name:34s} median {med:9.3f} ms  min {lo:9.3f} ms  "
          f"{nbytes / 1e9:8.2f} GB  {tbs:6.2f} TB/s", flush=True)
    out[name] = {"median_ms": med, "min_ms": lo, "bytes": nbytes, "tb_per_s": tbs}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=16384)
    p.add_argument("--d", type=int, default=1_000_000)
    p.add_argument("--csr-rows", type=int, default=1_000_000)
    p.add_argument("--csr-d", type=int, default=10_000_000)
    p.add_argument("--nnz-per-row", type=int, default=64)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=40)
    p.add_argument("--skip-dense", action="store_true")
    p.add_argument("--skip-csr", action="store_true")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("colstats_bench needs a GPU (no CPU fallback for timings)")
    dev = "cuda:0"
    res = {}

    if not args.skip_dense:
        shard, _ = generate_dense_problem(args.rows, args.d, seed=1234, device=dev,
                                          dtype=torch.bfloat16)
        n, d = shard.n, shard.d
        a_bytes = n * d * 2
        mult = torch.randn(n, device=dev, dtype=torch.float32)
        med, lo = timed(lambda: ops.dense_grad_from_mult(shard.features, mult),
                        args.warmup, args.reps)
        report("dense A^T.m pass (existing)", a_bytes + 4 * d, med, lo, res)
        med, lo = timed(lambda: column_stats(shard), args.warmup, args.reps)
        report("dense column_stats", a_bytes + 28 * d, med, lo, res)
        scaler = StandardScaler().fit(shard)
        med, lo = timed(lambda: scaler.transform(shard, inplace=True),
                        args.warmup, args.reps)
        report("dense transform(inplace)", 2 * a_bytes + 4 * d, med, lo, res)
        res["dense_colstats_over_grad"] = (
            res["dense column_stats"]["median_ms"]
            / res["dense A^T.m pass (existing)"]["median_ms"])
        print(f"dense column_stats / A^T.m pass = {res['dense_colstats_over_grad']:.2f}x",
              flush=True)
        del shard, mult, scaler
        torch.cuda.empty_cache()

    if not args.skip_csr:
        from sparkagd_amd.ops import hiplib

        shard, _ = generate_csr_problem(args.csr_rows, args.csr_d, args.nnz_per_row,
                                        seed=1234, device=dev)
        n, d, nnz = shard.n, shard.d, shard.nnz
        mult = torch.randn(n, device=dev, dtype=torch.float32)
        # CSC gradient: val + row per entry, colptr, grad out (mult gathers
        # ride the cache and are not counted)
        med, lo = timed(lambda: hiplib._csc_grad_skew(shard.csc, shard.csc_heavy,
                                                      mult, d),
                        args.warmup, args.reps)
        report("csr CSC gradient pass (existing)", 8 * nnz + 8 * d, med, lo, res)
        # statistics: val per entry, colptr, 28 B of results per column (the
        # zero folding re-reads colptr and the min/max vectors)
        med, lo = timed(lambda: column_stats(shard), args.warmup, args.reps)
        report("csr column_stats", 4 * nnz + 4 * d + 28 * d, med, lo, res)
        scaler = StandardScaler().fit(shard)
        # CSR val: val + col in, val out; CSC val: val in/out + colptr search
        med, lo = timed(lambda: scaler.transform(shard, inplace=True),
                        args.warmup, args.reps)
        report("csr transform(inplace)", 12 * nnz + 8 * nnz + 4 * d, med, lo, res)

    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
