#!/usr/bin/env python3
"""Feature scaling on ill-scaled data.

A planted logistic problem whose columns are multiplied by
``logspace(-spread, spread, d)`` — scales differing by orders of magnitude,
as real data has and the unit-scale generators do not. Trained twice with the
same iteration budget: on the raw columns, and with ``feature_scaling=True``
(per-column standardisation before optimising, weights mapped back to the
original space afterwards, as MLlib's GLM trainers do).

    python examples/train_scaled.py --n 2000 --d 64 --iters 20
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from sparkagd_amd import (  # noqa: E402
    DenseShard,
    LogisticRegressionWithAGD,
    column_stats,
    generate_dense_problem,
    ops,
)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=2000)
    p.add_argument("--d", type=int, default=64)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--spread", type=float, default=2.0,
                   help="column scales span 10^-spread .. 10^spread")
    args = p.parse_args()

    if torch.cuda.is_available():
        device, dtype = "cuda", torch.bfloat16
    else:
        device, dtype = "cpu", torch.float64

    base, _ = generate_dense_problem(args.n, args.d, seed=0, device=device,
                                     dtype=torch.float32)
    col_scale = torch.logspace(-args.spread, args.spread, args.d, device=device)
    shard = DenseShard((base.features * col_scale).to(dtype), base.labels)

    summary = column_stats(shard)
    print(f"column std: min {float(summary.std.min()):.3g}  "
          f"max {float(summary.std.max()):.3g}")

    kw = dict(num_iterations=args.iters, convergence_tol=0.0)
    raw = LogisticRegressionWithAGD.train(shard, **kw)
    scaled = LogisticRegressionWithAGD.train(shard, feature_scaling=True, **kw)

    print("iter   loss (raw columns)   loss (feature_scaling=True)")
    for i, (a, b) in enumerate(zip(raw.loss_history, scaled.loss_history), 1):
        print(f"{i:4d}   {a:18.6f}   {b:27.6f}")

    # the scaled model's weights are already in the original feature space
    _, lc = shard.eval(scaled.weights, ops.LOSS_LOGISTIC, need_grad=False)
    print(f"scaled model evaluated on the raw shard: loss {float(lc[0] / lc[1]):.6f}")
    print(f"final loss: raw {raw.loss_history[-1]:.6f}  "
          f"scaled {scaled.loss_history[-1]:.6f}")


if __name__ == "__main__":
    main()
