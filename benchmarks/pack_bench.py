#!/usr/bin/env python3
"""Packed vs raw bf16 shard on the flagship shape, in one process.

Builds the bench.py shard (same generator, same seed), times the one-time
pack, then runs the same AGD solve on the raw shard and on its packed copy
in alternation (W untimed + K timed iterations each, host clock between
device synchronises) and prints median/min ms per step for both, the pack
time and the break-even iteration count  pack_seconds / saving_per_step.

    python benchmarks/pack_bench.py [--rows 16384] [--d 1000000] [--rounds 5]
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

from sparkagd_amd import LogisticGradient, SquaredL2Updater, run  # noqa: E402
from sparkagd_amd.data import generate_dense_problem  # noqa: E402
from sparkagd_amd import ops  # noqa: E402


def timed_run(shard, warmup, steps, reg, d, dev):
    state = {}

    def hook(n_iter):
        if n_iter == warmup:
            torch.cuda.synchronize(dev)
            state["t0"] = time.perf_counter()
        if n_iter == warmup + steps:
            torch.cuda.synchronize(dev)
            state["t1"] = time.perf_counter()
            return "stop"
        return None

    w0 = torch.zeros(d, device=dev, dtype=torch.float32)
    w, hist = run(shard, LogisticGradient(), SquaredL2Updater(), 0.0,
                  warmup + steps, reg, w0, 1.0, math.inf, 0.5, 0.9, True,
                  loss_history_mode="backtrack", iteration_hook=hook,
                  pack_dense=False)  # the shard is packed (or not) by hand
    return (state["t1"] - state["t0"]) * 1e3 / steps, w, hist


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=16384)
    p.add_argument("--d", type=int, default=1_000_000)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--reg", type=float, default=1e-3)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    shard, _ = generate_dense_problem(a.rows, a.d, seed=1234,
                                      loss_type=ops.LOSS_LOGISTIC, device=dev,
                                      dtype=torch.bfloat16, label_noise=0.1)
    torch.cuda.synchronize(dev)
    pack_s = []
    for _ in range(3):
        shard.unpack()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ok = shard.pack()
        torch.cuda.synchronize(dev)
        pack_s.append(time.perf_counter() - t0)
        if not ok:
            raise SystemExit(f"pack refused: {shard.pack_refused}")
    pk = shard._packed
    ms = {"raw": [], "packed": []}
    out = {}
    for rnd in range(a.rounds + 1):  # first round untimed
        for way in ("raw", "packed"):
            if way == "raw":
                shard.unpack()
            else:
                shard.pack()
            t, w, hist = timed_run(shard, a.warmup, a.steps, a.reg, a.d, dev)
            out[way] = (w, hist)
            if rnd > 0:
                ms[way].append(t)
    res = {"rows": a.rows, "d": a.d, "warmup": a.warmup, "steps": a.steps,
           "rounds": a.rounds, "table": pk.table, "escapes": pk.nnz,
           "escape_fraction": pk.nnz / (a.rows * a.d),
           "packed_bytes": pk.nbytes, "raw_bytes": a.rows * a.d * 2,
           "pack_seconds_first": pack_s[0], "pack_seconds": min(pack_s)}
    for way in ms:
        res[way] = {"median_ms_per_step": statistics.median(ms[way]),
                    "min_ms_per_step": min(ms[way]),
                    "max_ms_per_step": max(ms[way])}
    saving = res["raw"]["median_ms_per_step"] - res["packed"]["median_ms_per_step"]
    res["break_even_iterations"] = (res["pack_seconds"] * 1e3 / saving
                                    if saving > 0 else None)
    (w_r, h_r), (w_p, h_p) = out["raw"], out["packed"]
    res["max_rel_loss_diff"] = max(abs(x - y) / max(abs(x), 1e-300)
                                   for x, y in zip(h_r, h_p))
    res["rel_weight_diff"] = float(torch.norm(w_p - w_r) / torch.norm(w_r))
    for way in ms:
        r = res[way]
        print(f"  {way:7s} median {r['median_ms_per_step']:8.3f} ms/step  "
              f"min {r['min_ms_per_step']:8.3f}  max {r['max_ms_per_step']:8.3f}")
    print(f"  pack {res['pack_seconds'] * 1e3:.1f} ms (first call "
          f"{res['pack_seconds_first'] * 1e3:.1f} ms), break-even "
          f"{res['break_even_iterations']}")
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
