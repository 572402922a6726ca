#!/usr/bin/env python3
"""Host-streamed bf16 shard: raw stream vs its 12-bit packed copy, one process.

Builds a randn bf16 shard in pinned host memory, then measures, raw and
packed in alternation (the first round untimed):

* the bare H2D copy loop over the same chunks (the ceiling of either stream),
* the one-time pack (first and later),
* one streamed ``eval`` pass (one H2D pass, two kernel passes per chunk),
* AGD ms/step (W untimed + K timed iterations, host clock between device
  synchronises),

and prints medians with min / max, the achieved H2D rates, the byte ratio,
the escape fraction, the break-even iteration count
pack_seconds / saving_per_step and the loss-history / weight differences of
the two ways. One JSON ``RESULT`` line at the end.

    python benchmarks/streaming_pack_bench.py [--rows 8192] [--d 1000000]
    python benchmarks/streaming_pack_bench.py --d 4096     # short rows, ~16 GB
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

from sparkagd_amd import (HostStreamedDenseShard, LogisticGradient,  # noqa: E402
                          SquaredL2Updater, ops, run)


def make_host_shard(n, d, dev, seed):
    """randn bf16 [n, d] in pinned host memory, generated on the device in
    row blocks (the host generator needs minutes at this size)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    feats = torch.empty((n, d), dtype=torch.bfloat16, pin_memory=True)
    block = max(1, min(n, (1 << 29) // d))
    w_true = torch.randn(d, generator=g, device=dev) / math.sqrt(d)
    labels = torch.empty(n, dtype=torch.float32, device=dev)
    for lo in range(0, n, block):
        hi = min(lo + block, n)
        x = torch.randn((hi - lo, d), generator=g, device=dev).to(torch.bfloat16)
        z = x.float() @ w_true
        flip = torch.rand(hi - lo, generator=g, device=dev) < 0.1
        labels[lo:hi] = ((z > 0) ^ flip).float()
        feats[lo:hi].copy_(x)
    torch.cuda.synchronize(dev)
    return feats, labels


def copy_loop_seconds(host, buf, chunk_rows, dev):
    n = host.shape[0]
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for lo in range(0, n, chunk_rows):
        hi = min(lo + chunk_rows, n)
        buf[: hi - lo].copy_(host[lo:hi], non_blocking=True)
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def eval_seconds(shard, w, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    _, lc = shard.eval(w, ops.LOSS_LOGISTIC)
    torch.cuda.synchronize(dev)
    t = time.perf_counter() - t0
    assert math.isfinite(float(lc[0]))
    return t


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
                  pack_dense=False)  # the shards are packed (or not) by hand
    return (state["t1"] - state["t0"]) / steps, w, hist


def spread(xs, scale=1.0):
    return {"median": statistics.median(xs) * scale, "min": min(xs) * scale,
            "max": max(xs) * scale}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=None,
                   help="default: 8192 at d = 10^6, else rows to about 16 GB")
    p.add_argument("--d", type=int, default=1_000_000)
    p.add_argument("--chunk-rows", type=int, default=None,
                   help="default: rows of about 2 GB of raw features")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--reg", type=float, default=1e-3)
    a = p.parse_args()
    if a.rounds < 5:
        raise SystemExit("--rounds must be at least 5")
    dev = torch.device("cuda", 0)
    n = a.rows or (8192 if a.d == 1_000_000 else (16 << 30) // (2 * a.d))
    d = a.d
    chunk = a.chunk_rows or max(1, min(n, (2 << 30) // (2 * d)))
    feats, labels = make_host_shard(n, d, dev, seed=11)
    raw = HostStreamedDenseShard(feats, labels, device=dev, chunk_rows=chunk)
    pk = HostStreamedDenseShard(feats, labels, device=dev, chunk_rows=chunk)
    assert pk.features_host.data_ptr() == raw.features_host.data_ptr()

    pack_s = []
    for _ in range(2):
        pk.unpack()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ok = pk.pack()
        torch.cuda.synchronize(dev)
        pack_s.append(time.perf_counter() - t0)
        if not ok:
            raise SystemExit(f"pack refused: {pk.pack_refused}")
    raw_bytes, packed_bytes = raw.streamed_nbytes, pk.streamed_nbytes
    side_bytes = sum(t.numel() * t.element_size() for esc, _ in pk._pack_esc
                     for t in esc.values() if t is not None)

    w = torch.zeros(d, device=dev)
    ways = {"raw": (raw, raw.features_host, raw._buf[0], raw_bytes),
            "packed": (pk, pk._packed_host, pk._pbuf[0], packed_bytes)}
    copy_s = {k: [] for k in ways}
    eval_s = {k: [] for k in ways}
    step_s = {k: [] for k in ways}
    out = {}
    for rnd in range(a.rounds + 1):  # first round untimed
        for way, (shard, host, buf, _) in ways.items():
            tc = copy_loop_seconds(host, buf, chunk, dev)
            te = eval_seconds(shard, w, dev)
            ts, w_end, hist = timed_run(shard, a.warmup, a.steps, a.reg, d, dev)
            out[way] = (w_end, hist)
            if rnd > 0:
                copy_s[way].append(tc)
                eval_s[way].append(te)
                step_s[way].append(ts)

    res = {"rows": n, "d": d, "chunk_rows": chunk, "warmup": a.warmup,
           "steps": a.steps, "rounds": a.rounds, "table": pk._pack_table,
           "escapes": pk._pack_nnz, "escape_fraction": pk._pack_nnz / (n * d),
           "side_list_bytes": side_bytes,
           "raw_streamed_nbytes": raw_bytes, "packed_streamed_nbytes": packed_bytes,
           "streamed_nbytes_ratio": packed_bytes / raw_bytes,
           "pack_seconds_first": pack_s[0], "pack_seconds": min(pack_s[1:])}
    for way, (_, _, _, nbytes) in ways.items():
        r = {"h2d_ceiling_ms": spread(copy_s[way], 1e3),
             "eval_ms": spread(eval_s[way], 1e3),
             "agd_ms_per_step": spread(step_s[way], 1e3)}
        r["h2d_ceiling_gbps"] = nbytes / statistics.median(copy_s[way]) / 1e9
        r["eval_h2d_gbps"] = nbytes / statistics.median(eval_s[way]) / 1e9
        res[way] = r
    for key in ("eval_ms", "agd_ms_per_step"):
        res[f"{key}_ratio"] = res["packed"][key]["median"] / res["raw"][key]["median"]
    saving = (res["raw"]["agd_ms_per_step"]["median"]
              - res["packed"]["agd_ms_per_step"]["median"])
    for key in ("pack_seconds_first", "pack_seconds"):
        res[f"break_even_iterations_{key[5:]}"] = (
            res[key] * 1e3 / saving if saving > 0 else None)
    (w_r, h_r), (w_p, h_p) = out["raw"], out["packed"]
    res["max_rel_loss_diff"] = max(abs(x - y) / max(abs(x), 1e-300)
                                   for x, y in zip(h_r, h_p))
    res["rel_weight_diff"] = float(torch.norm(w_p - w_r) / torch.norm(w_r))

    print(f"shard {n} x {d} bf16, {raw_bytes / 1e9:.2f} GB raw, "
          f"{packed_bytes / 1e9:.2f} GB packed "
          f"({res['streamed_nbytes_ratio']:.4f}x), chunks of {chunk} rows, "
          f"{res['escapes']} escapes ({res['escape_fraction']:.2e}), "
          f"side lists {side_bytes / 1e6:.1f} MB")
    for way in ways:
        r = res[way]
        print(f"  {way:7s} H2D loop {r['h2d_ceiling_ms']['median']:8.1f} ms "
              f"({r['h2d_ceiling_gbps']:.1f} GB/s)  eval "
              f"{r['eval_ms']['median']:8.1f} ms [{r['eval_ms']['min']:.1f}, "
              f"{r['eval_ms']['max']:.1f}] ({r['eval_h2d_gbps']:.1f} GB/s)  AGD "
              f"{r['agd_ms_per_step']['median']:8.1f} ms/step "
              f"[{r['agd_ms_per_step']['min']:.1f}, {r['agd_ms_per_step']['max']:.1f}]")
    print(f"  packed / raw: eval {res['eval_ms_ratio']:.4f}, AGD step "
          f"{res['agd_ms_per_step_ratio']:.4f} (bytes {res['streamed_nbytes_ratio']:.4f})")
    print(f"  pack {res['pack_seconds'] * 1e3:.0f} ms (first call "
          f"{res['pack_seconds_first'] * 1e3:.0f} ms), break-even "
          f"{res['break_even_iterations_seconds']} iterations "
          f"(first call: {res['break_even_iterations_seconds_first']})")
    print(f"  loss history max rel diff {res['max_rel_loss_diff']:.3e}, "
          f"weights rel diff {res['rel_weight_diff']:.3e}")
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
