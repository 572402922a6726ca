#!/usr/bin/env python3
"""k-fold cross-validation of a regularisation sweep in one training run.

All (lambda, fold) models train as the columns of one weight block, so each
pass over the shard serves every one of them:

    python examples/cross_validate.py --n 20000 --d 256
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from sparkagd_amd import (  # noqa: E402
    AGDConfig,
    LogisticGradient,
    cross_validate,
    generate_dense_problem,
)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=20000)
    p.add_argument("--d", type=int, default=256)
    p.add_argument("--iters", type=int, default=40)
    p.add_argument("--folds", type=int, default=3)
    p.add_argument("--lambdas", type=float, nargs="+",
                   default=[1e-4, 1e-3, 1e-2, 1e-1])
    args = p.parse_args()

    if torch.cuda.is_available():
        device, dtype = "cuda", torch.bfloat16
    else:
        device, dtype = "cpu", torch.float64
    # label noise makes the sweep matter: too little regularisation overfits
    shard, _ = generate_dense_problem(args.n, args.d, seed=7, device=device,
                                      dtype=dtype, label_noise=1.0)

    res = cross_validate(
        shard, args.lambdas, n_folds=args.folds, gradient=LogisticGradient(),
        num_iterations=args.iters,
        config=AGDConfig(loss_history_mode="backtrack"))

    print(f"{len(args.lambdas)} lambdas x {args.folds} folds = "
          f"{len(args.lambdas) * args.folds} models in one run "
          f"({len(res.loss_history)} iterations)")
    for lam, mean, std in zip(res.lambdas, res.mean_loss.tolist(),
                              res.std_loss.tolist()):
        print(f"lambda={lam:<8g} held-out loss {mean:.5f} +- {std:.5f}")
    print(f"best lambda: {res.best_lambda:g}")
    print(f"refit model: {res.model.weights.numel()} weights, "
          f"{len(res.model.loss_history)} iterations")


if __name__ == "__main__":
    main()
