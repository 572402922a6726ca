"""Packed bf16 stream, the tails: the packed margins kernel at every row-group
and sweep-count tail against the raw path (bit-identical without escapes) and
a float64 oracle (with escapes), and the encoder's one-bit-per-group escape
words and side lists against the CPU reference on hand-built escapes."""

import math

import numpy as np
import pytest
import torch

from sparkagd_amd import ops, packing
from sparkagd_amd.data import DenseShard, InterceptShard
from test_dense_pack import (bf16_bits, bits_to_bf16, few_binade_features,
                             ref_encode, ref_table)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# n: row-group tails for 4 and for 8 rows per wave. d: zero, one, two and odd
# counts of whole 64-group sweeps (d = 512 k), each with and without a partial
# last sweep. The last two shapes split the columns into slabs and end on a
# tail row group.
ROWS = [1, 3, 4, 5, 7, 8, 9, 15, 17]
COLS = [8, 504, 512, 520, 1024, 1032, 1544]
SHAPES = [(n, d) for d in COLS for n in ROWS] + [(5, 65536), (9, 131072)]


def _vectors(n, d, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    y = (torch.randn(n, generator=g, device=DEV) > 0).to(torch.float32)
    w = torch.randn(d, generator=g, device=DEV) / math.sqrt(d)
    return y, w


def _pair(x, y):
    raw = DenseShard(x.to(DEV), y)
    pk = DenseShard(x.to(DEV).clone(), y)
    assert pk.pack(), pk.pack_refused
    return raw, pk


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def clean_case(request):
    n, d = request.param
    x = few_binade_features(n, d, seed=7 * n + d)
    y, w = _vectors(n, d, seed=d + n)
    raw, pk = _pair(x, y)
    assert pk._packed.nnz == 0
    return raw, pk, w


def test_margins_bit_identical_to_raw(clean_case):
    raw, pk, w = clean_case
    assert torch.equal(pk.margins(w), raw.margins(w))


def test_eval_from_margins_bit_identical_to_raw(clean_case):
    raw, pk, w = clean_case
    z = pk.margins(w)
    g_r, lc_r = raw.eval_from_margins(z, ops.LOSS_LOGISTIC)
    g_p, lc_p = pk.eval_from_margins(z, ops.LOSS_LOGISTIC)
    assert torch.equal(g_p, g_r) and torch.equal(lc_p, lc_r)
    # the fused evaluation runs the margins kernel itself
    g_r2, lc_r2 = raw.eval(w, ops.LOSS_LOGISTIC)
    g_p2, lc_p2 = pk.eval(w, ops.LOSS_LOGISTIC)
    assert torch.equal(g_p2, g_r2) and torch.equal(lc_p2, lc_r2)


def test_intercept_shard_bit_identical_to_raw(clean_case):
    raw, pk, w = clean_case
    wb = torch.cat([w, torch.tensor([0.25], device=DEV)])
    ir, ip = InterceptShard(raw), InterceptShard(pk)
    assert torch.equal(ip.margins(wb), ir.margins(wb))
    g_r, lc_r = ir.eval(wb, ops.LOSS_LOGISTIC)
    g_p, lc_p = ip.eval(wb, ops.LOSS_LOGISTIC)
    assert torch.equal(g_p, g_r) and torch.equal(lc_p, lc_r)


# --- margins with escapes ----------------------------------------------------

@pytest.mark.parametrize("n,d", [(37, 1544), (9, 65536)])
def test_margins_with_escapes_match_f64_oracle(n, d):
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(3 * n + d))
    x = x.to(torch.bfloat16)
    x[0, 0] = 2.0 ** -30
    x[n // 2, d // 2] = 2.0 ** -30
    x[n - 1, d - 1] = 2.0 ** 20
    x[1, 8] = -(2.0 ** 20)
    y, w = _vectors(n, d, seed=d + 1)
    # keeps |z| = O(1) (f32 margins carry ulp(|z|)) while each planted escape
    # still moves its margin by 4
    w[d - 1] = 2.0 ** -18
    w[8] = -(2.0 ** -18)
    pk = DenseShard(x.to(DEV), y)
    assert pk.pack(), pk.pack_refused
    assert pk._packed.nnz >= 4
    z = pk.margins(w)
    ref = x.to(DEV).double() @ w.double()
    torch.testing.assert_close(z.double(), ref, rtol=2e-4, atol=2e-3)
    assert torch.equal(pk.margins(w), z)  # run to run


# --- encoder -------------------------------------------------------------------

BASE_HIGHS = [0x00, 0x3B, 0x3C, 0x3D, 0x3E, 0x3F, 0x40, 0x41]


def _hand_built(groups):
    """8 rows of d = 8 * groups: row 0 has no escape, row 1 nothing but
    escapes, row 2 escapes in its first and last group and in the groups on
    both sides of every 64-group boundary (one or two per group), row 3 one
    escape in every group; the rest are clean. Clean elements cycle through
    BASE_HIGHS, escapes through 48 other high bytes, so the histogram's top
    eight are BASE_HIGHS whatever the shape."""
    n, d = 8, 8 * groups
    r = np.arange(n)[:, None]
    c = np.arange(d)[None, :]
    high = np.asarray(BASE_HIGHS)[(c + r) % 8]
    esc_high = 0x01 + (c * 7 + r * 13) % 48   # 0x01..0x30: none is a base high
    esc = np.zeros((n, d), dtype=bool)
    esc[1, :] = True
    for g in range(groups):
        if g in (0, groups - 1) or g % 64 in (0, 63):
            esc[2, g * 8 + (np.array([0, 7]) if g % 2 == 0 else np.array([3]))] = True
        esc[3, g * 8 + g % 8] = True
    low = (c * 37 + r * 11) & 0xFF
    sign = (c + r // 2) & 1
    bits = (sign << 15) | (np.where(esc, esc_high, high) << 8) | low
    return bits.astype(np.uint16), esc


@pytest.mark.parametrize("groups", [1, 63, 64, 65, 193])
def test_encoder_hand_built_escapes(groups, monkeypatch):
    # the cap is policy, not format
    monkeypatch.setattr(packing, "PACK_ESCAPE_CAP", 1.0)
    bits, esc = _hand_built(groups)
    n, d = bits.shape
    table = ref_table(bits)
    assert table == BASE_HIGHS
    packed_ref, esc_ref = ref_encode(bits, table)
    assert np.array_equal(esc_ref, esc)
    x = bits_to_bf16(bits).to(DEV)

    # the encode pass itself: bytes, per-row counts, one bit per group
    lo, hi = packing.table_luts(table)
    hip = ops._get_hip()
    packed, esc_count, words = hip.dense_pack_encode(x, lo, hi)
    assert np.array_equal(packed.cpu().numpy(), packed_ref)
    assert np.array_equal(esc_count.cpu().numpy(), esc.sum(1))
    gs = packed_ref.shape[1] // 12
    assert tuple(words.shape) == (n, -(-gs // 64))
    any_esc = np.zeros((n, words.shape[1] * 64), dtype=bool)
    any_esc[:, :groups] = esc.reshape(n, groups, 8).any(2)
    got = words.cpu().numpy().view(np.uint64)
    got = (got[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    assert np.array_equal(got.reshape(n, -1).astype(bool), any_esc)

    # the whole pack: side lists in row and in column order
    s = DenseShard(x, torch.zeros(n, device=DEV))
    assert s.pack(), s.pack_refused
    pk = s._packed
    assert pk.table == table and pk.nnz == int(esc.sum())
    assert np.array_equal(pk.packed.cpu().numpy(), packed_ref)
    rowptr = pk.esc["rowptr"].cpu().numpy()
    assert np.array_equal(np.diff(rowptr), esc.sum(1)) and rowptr[0] == 0
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    cols = pk.esc["col"].cpu().numpy()
    assert np.array_equal(np.argwhere(esc), np.stack([rows, cols], 1))
    xf = x.cpu().float()
    assert torch.equal(pk.esc["val"].cpu().view(torch.int32),
                       xf[torch.from_numpy(esc)].view(torch.int32))
    colptr = pk.esc["colptr"].cpu().numpy()
    assert np.array_equal(np.diff(colptr), esc.sum(0)) and colptr[0] == 0
    ccols = np.repeat(np.arange(d), np.diff(colptr))
    crow = pk.esc["row"].cpu().numpy()
    assert np.array_equal(np.argwhere(esc.T), np.stack([ccols, crow], 1))
    assert torch.equal(pk.esc["cval"].cpu().view(torch.int32),
                       xf[crow, ccols].view(torch.int32))

    # and back, bit for bit
    assert np.array_equal(bf16_bits(hip.dense_pack_decode(pk)), bits)
