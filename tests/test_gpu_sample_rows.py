"""Row-sampled mini-batch passes (csrc/agd_rows.hip) against the exact f64
oracle: on the data of ``exact_oracle`` every summation order gives the one
result, so the gradient, ``loss_count`` and the compact multiplier are
compared with ``torch.equal`` and a lost row, slab or column cannot hide."""

import math

import pytest
import torch

import exact_oracle as xo
from exact_oracle import HINGE, LSQ, exact_equal
from sparkagd_amd import (DenseShard, InterceptShard, LogisticGradient,
                          SimpleUpdater, ops,
                          run_mini_batch)
from sparkagd_amd.data import generate_dense_problem

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ["bf16", "f32", "f64", "fp8"]


def _shape(case, name):
    """(n, d, forced n_slabs, forced n_rb) of a case. W is the 16-byte lane
    load width, R the rows of a wave (4, fp8 8)."""
    w = xo.W_FULL[name]
    return {
        # list shorter than R; one double sweep and one single sweep
        "short": (3, 3 * 64 * w, None, None),
        # list length % R != 0 (23 rows), d % W != 0: the W = 1 loads
        "tail": (37, 1027, None, None),
        # three column slabs (the last one 24 columns) and four row blocks
        # over a list of 45 / 37 / 46 rows: uneven blocks
        "slabs": (70, 2 * 64 * w + 24, 3, 4),
        "zeros": (9, 3 * 64 * w, None, None),
        "ones": (9, 3 * 64 * w, None, None),
        # the unsampled rows hold NaN / inf: nothing outside the list is read
        "poison": (70, 2 * 64 * w + 24, None, None),
    }[case]


@pytest.mark.parametrize("weights", [False, True], ids=["plain", "weights"])
@pytest.mark.parametrize("loss", [LSQ, HINGE], ids=["lsq", "hinge"])
@pytest.mark.parametrize("case", ["short", "tail", "slabs", "zeros", "ones",
                                  "poison"])
@pytest.mark.parametrize("name", NAMES)
def test_dense_eval_rows_exact(name, case, loss, weights):
    n, d, n_slabs, n_rb = _shape(case, name)
    p = xo.dense_problem(n, d, name)
    mask = {"zeros": torch.zeros_like(p.mask),
            "ones": torch.ones_like(p.mask)}.get(case, p.mask)
    sw = p.sw if weights else None
    g64, lc64, m64 = xo.dense_eval64(p, loss, mask=mask, sw=sw)
    A = p.A
    if case == "poison":
        A = xo.poison_rows(p, torch.nonzero(mask == 0).reshape(-1).tolist())[1]
    g, lc, (rows, count, mult) = ops.dense_eval_rows(
        A.to(DEV), p.y.to(DEV), p.w.to(DEV), loss, mask.to(DEV), True,
        None if sw is None else sw.to(DEV), n_slabs, n_rb, return_state=True)
    listed = torch.nonzero(mask).reshape(-1)
    assert int(count) == listed.numel()
    assert torch.equal(rows[:listed.numel()].cpu().long(), listed)
    assert exact_equal(mult[:listed.numel()], m64[listed])
    assert exact_equal(lc, lc64), (lc, lc64)
    assert exact_equal(g, g64)
    if case == "zeros":
        assert not g.any() and lc.tolist() == [0.0, 0.0]


@pytest.mark.parametrize("n", [1, 4095, 4097, 256 * 4096 + 5])
def test_compact_rows(n):
    """One thread's scalar tail, one block less a byte, a second block, and
    more blocks than the one-block scan has threads."""
    from sparkagd_amd.ops import hiplib

    gen = torch.Generator().manual_seed(n)
    mask = (torch.rand(n, generator=gen) < 0.3).to(torch.uint8)
    mask[0] = mask[n - 1] = 1
    rows, count = hiplib.compact_rows(mask.to(DEV))
    listed = torch.nonzero(mask).reshape(-1)
    assert int(count) == listed.numel()
    assert torch.equal(rows[:listed.numel()].cpu().long(), listed)


def test_sgd_sample_rows_end_to_end(monkeypatch):
    """20 SGD steps at f = 0.25 on a 512 x 256 f32 logistic problem against
    the same run in f64. The f64 run is plain torch on the same device
    (SPARKAGD_FORCE_REFERENCE), so that the seeded device masks, and with
    them the batches, are the same.

    Measured deviation of the final weights (max abs) and of the loss history
    (max rel) from the f64 run on the MI355X:
        masked path (sample_rows=False): 4.08e-08, 3.09e-08
        list path   (sample_rows=True):  4.08e-08, 2.44e-08
    The list path differs from the masked one only in f32 summation order
    and is allowed twice the masked path's deviation."""
    MASKED_W, MASKED_H = 4.08e-08, 3.09e-08  # measured, see above
    shard, _ = generate_dense_problem(512, 256, seed=3, device=DEV,
                                      dtype=torch.float32)
    w0 = torch.zeros(256, device=DEV)
    args = (LogisticGradient(), SimpleUpdater(), 1.0, 20, 0.0, 0.25)
    w_def, h_def = run_mini_batch(shard, *args, w0)
    w_off, h_off = run_mini_batch(shard, *args, w0, sample_rows=False)
    w_on, h_on = run_mini_batch(shard, *args, w0, sample_rows=True)
    # the default run is the masked path, bit for bit
    assert torch.equal(w_def, w_off) and h_def == h_off
    monkeypatch.setenv("SPARKAGD_FORCE_REFERENCE", "1")
    shard64 = DenseShard(shard.features.double(), shard.labels)
    w64, h64 = run_mini_batch(shard64, *args, w0.double())
    monkeypatch.delenv("SPARKAGD_FORCE_REFERENCE")

    def dev(w, h):
        return (float((w.double() - w64).abs().max()),
                max(abs(a - b) / abs(b) for a, b in zip(h, h64)))

    # with an intercept: the masked composition against the list one; both
    # sum at most 512 f32 terms per entry, so they differ by less than
    # 512 * 2^-24 of the largest entry
    ish = InterceptShard(shard)
    wb = torch.cat([w_off, torch.full((1,), 0.5, device=DEV)])
    mask = (torch.arange(512, device=DEV) % 4 == 1).to(torch.uint8)
    g0, lc0 = ish.eval(wb, ops.LOSS_LOGISTIC, mask)
    g1, lc1 = ish.eval(wb, ops.LOSS_LOGISTIC, mask, sample_rows=0.25)
    assert g1.shape == g0.shape == (257,) and float(lc1[1]) == float(lc0[1])
    assert float((g1 - g0).abs().max()) <= 512 * 2 ** -24 * float(g0.abs().max())
    assert float(lc1[0]) == pytest.approx(float(lc0[0]), rel=512 * 2 ** -24)

    (mw, mh), (lw, lh) = dev(w_off, h_off), dev(w_on, h_on)
    print(f"masked: w {mw:.3g} hist {mh:.3g}; list: w {lw:.3g} hist {lh:.3g}")
    assert len(h_on) == len(h64) == 20 and math.isfinite(h_on[-1])
    assert lw <= 2 * MASKED_W and lh <= 2 * MASKED_H
