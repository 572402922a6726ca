#!/usr/bin/env python3
"""Evaluation metrics pass: the fused HIP kernel next to what it replaces, on
one MI355X at n = 1e7 margins, B = 1000 bins.

    fused              ops.binary_metrics (k_binary_metrics + its two one-block
                       reduces): histograms, confusion, seven f64 sums, NaN
                       count, one pass over margins and labels
    fused weighted     the same with f32 sample weights (2^-32 fixed point)
    torch composition  the same outputs from torch ops on the GPU: bucketize,
                       two bincounts, comparisons for the confusion, softplus
                       and squared / absolute error sums in f64, isnan count
    roc_auc (argsort)  evaluation.roc_auc, the f64 argsort + unique path that
                       was the only AUC before

The three are timed in alternation (one of each per round) with device events
around --inner back-to-back calls, after --warmup rounds; the figures are the
median and minimum per call over --reps rounds. GB/s is the bytes the fused
pass must read (margins + labels [+ weights]) over its median time. Needs a
GPU: there is no CPU fallback for a timing.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sparkagd_amd import evaluation, ops  # noqa: E402
from sparkagd_amd.evaluation import _edges_for  # noqa: E402


def torch_composition(z, y, edges, cut):
    """binary_metrics' outputs from stock torch ops (unweighted)."""
    nb = edges.numel() + 1
    pos = y > 0.5
    bins = torch.bucketize(z, edges, right=True)
    hist_pos = torch.bincount(torch.where(pos, bins, nb), minlength=nb + 1)[:nb]
    hist_neg = torch.bincount(torch.where(pos, nb, bins), minlength=nb + 1)[:nb]
    pred = z > cut
    conf = torch.stack([(pos & pred).sum(), (~pos & pred).sum(),
                        (pos & ~pred).sum(), (~pos & ~pred).sum()])
    zd, yd = z.double(), y.double()
    sp = torch.nn.functional.softplus
    diff = zd - yd
    sums = torch.stack([
        torch.full((), float(z.numel()), dtype=torch.float64, device=z.device),
        torch.where(pos, sp(-zd), sp(zd)).sum(), (diff * diff).sum(),
        diff.abs().sum(), yd.sum(), (yd * yd).sum(), diff.sum()])
    return hist_pos, hist_neg, conf, sums, torch.isnan(z).sum()


def timed_alternating(fns, warmup, reps, inner):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(inner):
                fn()
            t1.record()
            t1.synchronize()
            ms[name].append(t0.elapsed_time(t1) / inner)
    return {k: (statistics.median(v), min(v)) for k, v in ms.items()}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=10_000_000)
    p.add_argument("--bins", type=int, default=1000)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--inner", type=int, default=10)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs a GPU (no CPU fallback for timings)")
    dev = "cuda:0"
    n = args.n
    g = torch.Generator(device=dev).manual_seed(1234)
    z = torch.randn(n, generator=g, device=dev) * 4
    y = (torch.rand(n, generator=g, device=dev) < torch.sigmoid(z)).float()
    w = torch.rand(n, generator=g, device=dev) * 4
    edges = _edges_for(args.bins, None, torch.float32).to(dev)

    # same answers first: the integers exactly, the sums to f64 rounding
    fused = ops.binary_metrics(z, y, edges, 0.0)
    comp = torch_composition(z, y, edges, 0.0)
    for a, b in zip(fused[:3], comp[:3]):
        assert torch.equal(a, b)
    torch.testing.assert_close(fused[3], comp[3], rtol=1e-8, atol=0)
    auc_sorted = evaluation.roc_auc(z, y)

    fns = {
        "fused": lambda: ops.binary_metrics(z, y, edges, 0.0),
        "fused weighted": lambda: ops.binary_metrics(z, y, edges, 0.0, w),
        "torch composition": lambda: torch_composition(z, y, edges, 0.0),
        "roc_auc (argsort)": lambda: evaluation.roc_auc(z, y),
    }
    times = timed_alternating(fns, args.warmup, args.reps, args.inner)
    res = {"n": n, "bins": args.bins, "auc_argsort": auc_sorted}
    nbytes = {"fused": 8 * n, "fused weighted": 12 * n}
    for name, (med, lo) in times.items():
        line = f"{name:20s} median {med:9.4f} ms  min {lo:9.4f} ms"
        res[name] = {"median_ms": med, "min_ms": lo}
        if name in nbytes:
            gbs = nbytes[name] / (med * 1e-3) / 1e9
            res[name]["gb_per_s"] = gbs
            line += f"  {nbytes[name] / 1e6:7.1f} MB  {gbs:8.1f} GB/s"
        print(line, flush=True)
    res["composition_over_fused"] = (times["torch composition"][0]
                                     / times["fused"][0])
    res["argsort_over_fused"] = times["roc_auc (argsort)"][0] / times["fused"][0]
    print(f"torch composition / fused = {res['composition_over_fused']:.2f}x, "
          f"roc_auc argsort / fused = {res['argsort_over_fused']:.2f}x", flush=True)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
