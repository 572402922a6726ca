#!/usr/bin/env python3
"""Mini-batch SGD step time with the masked passes and with the row-sampled
list passes (``run_mini_batch(..., sample_rows=True)``), on one MI355X.

Two bf16 shapes, logistic loss: the flagship 16384 x 1e6 and a tall
1e6 x 10240. For each fraction f in {1.0, 0.1, 0.01} the two ways are run in
alternation in this one process, one of each per round after one untimed
round; a timed unit is one run_mini_batch of --steps steps bracketed by
device synchronises (every step ends in a host fetch of its loss). The
figures are the median, minimum and maximum ms/step over --rounds rounds.
``sample_rows=False`` is the yardstick: it is the path of the parent commit.

Per pass, the stream rate over the bytes of the *sampled* rows (f * n * d *
2 bytes) is printed next to the rate of the full pass over the whole shard:
the margins side is one loss-only evaluation (compaction, A.w, multiplier),
the gradient side the difference to a full evaluation, both by device events
over --reps calls. Needs a GPU: there is no CPU fallback for a timing.
"""

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sparkagd_amd import LogisticGradient, SimpleUpdater, ops, run_mini_batch  # noqa: E402
from sparkagd_amd.data import generate_dense_problem  # noqa: E402

DEV = "cuda:0"
FRACTIONS = (1.0, 0.1, 0.01)


def sgd_ms_per_step(shard, f, sample_rows, steps):
    w0 = torch.zeros(shard.d, device=DEV, dtype=torch.float32)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_mini_batch(shard, LogisticGradient(), SimpleUpdater(), 1.0, steps, 0.0,
                   f, w0, sample_rows=sample_rows)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))


def pass_rates(shard, f, reps):
    """TB/s of the margins side and of the gradient side: the full passes
    over all bytes, the list passes over the sampled bytes."""
    w = torch.full((shard.d,), 1e-3, device=DEV)
    A, y = shard.features, shard.labels
    gen = torch.Generator(device=DEV).manual_seed(7)
    mask = (torch.rand(shard.n, generator=gen, device=DEV) < f).to(torch.uint8)
    nbytes = A.numel() * A.element_size()
    sampled = int(mask.sum()) * shard.d * A.element_size()
    out = {}
    for tag, fn, b in (
            ("full", lambda g: ops.dense_eval(A, y, w, 0, None, g), nbytes),
            ("list", lambda g: ops.dense_eval_rows(
                A, y, w, 0, mask, g, expected_rows=int(f * shard.n) + 1), sampled)):
        t_m = event_ms(lambda: fn(False), reps)
        t_all = event_ms(lambda: fn(True), reps)
        out[tag] = {"margins_ms": t_m, "grad_ms": t_all - t_m,
                    "margins_TBps": b / t_m / 1e9,
                    "grad_TBps": b / (t_all - t_m) / 1e9}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16384x1000000,1000000x10240")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.hip_available(), "needs the GPU"
    for shape in args.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        shard, _ = generate_dense_problem(n, d, seed=11, device=DEV,
                                          dtype=torch.bfloat16)
        for f in FRACTIONS:
            ms = {False: [], True: []}
            for rnd in range(args.rounds + 1):
                for way in (False, True):
                    t = sgd_ms_per_step(shard, f, way, args.steps)
                    if rnd:
                        ms[way].append(t)
            res = {"shape": shape, "dtype": "bf16", "fraction": f,
                   "steps": args.steps, "rounds": args.rounds}
            for way, tag in ((False, "masked"), (True, "sample_rows")):
                res[tag + "_ms_per_step"] = {
                    "median": statistics.median(ms[way]), "min": min(ms[way]),
                    "max": max(ms[way])}
            if f < 1.0:
                res["passes"] = pass_rates(shard, f, args.reps)
            print(json.dumps(res), flush=True)
        del shard
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
