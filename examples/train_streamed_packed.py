#!/usr/bin/env python3
"""Train on a host-streamed bf16 shard that streams its lossless 12-bit
packed copy: 0.75x the bytes over the host link per pass, and with
``release_raw=True`` 0.75x the host memory.

    python examples/train_streamed_packed.py [--device cuda]
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from sparkagd_amd import (HostStreamedDenseShard, LogisticGradient,  # noqa: E402
                          SquaredL2Updater, run)
from sparkagd_amd.data import generate_dense_problem  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=4096)
    p.add_argument("--d", type=int, default=1024)
    p.add_argument("--iters", type=int, default=15)
    p.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    a = p.parse_args()
    dense, _ = generate_dense_problem(a.n, a.d, seed=0, dtype=torch.bfloat16)
    shard = HostStreamedDenseShard(dense.features, dense.labels,
                                   device=a.device, chunk_rows=1024)
    if not shard.pack(release_raw=True):
        print(f"not packed ({shard.pack_refused}): streaming the raw features")
    print(f"packed={shard.is_packed} in {shard.pack_seconds or 0.0:.3f} s; one pass "
          f"streams {shard.streamed_nbytes} of {shard.nbytes} logical bytes")
    w0 = torch.zeros(a.d, device=a.device)
    w, history = run(shard, LogisticGradient(), SquaredL2Updater(), 0.0,
                     a.iters, 1e-3, w0, pack_dense=False)  # packed by hand
    print(f"loss {history[0]:.4f} -> {history[-1]:.4f} in {len(history)} iterations")
    shard.unpack()  # the raw pinned features again, bit for bit
    assert torch.equal(shard.features_host.view(torch.int16),
                       dense.features.view(torch.int16))


if __name__ == "__main__":
    main()
