#!/usr/bin/env python3
"""Train, then score and evaluate whole shards — no feature copy, no argsort.

Three problems, each evaluated on the shard it was trained on through
``evaluate`` (one fused metrics pass on the GPU, the plain-torch oracle on
CPU):

* a CSR logistic shard with per-example sample weights -> ``BinaryMetrics``
* a dense least-squares shard                           -> ``RegressionMetrics``
* a dense softmax shard                                 -> ``MulticlassMetrics``

    python examples/evaluate_sharded.py --n 4000 --iters 20

Exits non-zero if a metric is implausible for a planted problem.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from sparkagd_amd import (  # noqa: E402
    LinearRegressionWithAGD,
    LogisticRegressionWithAGD,
    SoftmaxRegressionWithAGD,
    evaluate,
    generate_dense_problem,
    generate_multiclass_problem,
    ops,
)
from sparkagd_amd.data import generate_csr_problem  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=4000)
    p.add_argument("--d", type=int, default=64)
    p.add_argument("--classes", type=int, default=5)
    p.add_argument("--iters", type=int, default=20)
    args = p.parse_args()

    if torch.cuda.is_available():
        device, dtype = "cuda", torch.bfloat16
    else:
        device, dtype = "cpu", torch.float32
    problems = []

    # sparse, weighted, binary
    csr, _ = generate_csr_problem(args.n, 50 * args.d, 16, seed=0, device=device)
    g = torch.Generator().manual_seed(0)
    csr.sample_weight = (0.5 + torch.rand(args.n, generator=g)).to(device)
    model = LogisticRegressionWithAGD.train(csr, num_iterations=args.iters)
    m = evaluate(model, csr, num_bins=200)
    _, best_f1 = (t.max() for t in m.f_measure_by_threshold())
    print(f"CSR logistic   n={m.count:.1f} (weighted)  AUC {m.area_under_roc:.4f}  "
          f"AUPR {m.area_under_pr:.4f}  accuracy {m.accuracy:.4f}  "
          f"F1 {m.f1:.4f} (best over thresholds {float(best_f1):.4f})  "
          f"log-loss {m.log_loss:.4f}")
    pred = model.predict_shard(csr)
    print(f"               predict_shard: {int(pred.sum())} of {csr.n} rows positive")
    problems += [m.area_under_roc < 0.8, m.accuracy < 0.7, m.log_loss > 0.69,
                 float(best_f1) < m.f1 - 1e-12]

    # dense regression
    dense, _ = generate_dense_problem(args.n, args.d, seed=1, device=device,
                                      dtype=dtype, loss_type=ops.LOSS_LEAST_SQUARES)
    model = LinearRegressionWithAGD.train(dense, num_iterations=args.iters)
    m = evaluate(model, dense)
    print(f"dense lsq      n={m.count:.0f}  RMSE {m.rmse:.4f}  MAE {m.mae:.4f}  "
          f"R2 {m.r2:.4f}  explained variance {m.explained_variance:.4f}")
    problems += [not m.r2 > 0.5, not m.explained_variance >= m.r2 - 1e-9]

    # dense multiclass
    multi, _ = generate_multiclass_problem(args.n, args.d, args.classes, seed=2,
                                           device=device, dtype=dtype)
    model = SoftmaxRegressionWithAGD.train(multi, args.classes,
                                           num_iterations=args.iters)
    m = evaluate(model, multi)
    print(f"dense softmax  n={m.count:.0f}  accuracy {m.accuracy:.4f}  "
          f"weighted F1 {m.weighted_f1:.4f}  log-loss {m.log_loss:.4f}")
    print("               recall per class: "
          + " ".join(f"{m.recall(k):.3f}" for k in range(args.classes)))
    problems += [m.accuracy < 2.0 / args.classes,
                 abs(m.weighted_recall - m.accuracy) > 1e-9]

    if any(problems):
        print(f"implausible metrics: checks {problems}", file=sys.stderr)
        return 1
    print("evaluation OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
