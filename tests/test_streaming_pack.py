"""Host-streamed bf16 shard with the 12-bit packed host copy (CPU tier).

The CPU shard has no packed kernel: it decodes each packed chunk with
packing.decode_torch and runs the ordinary ops, so every result must equal
the unpacked streamed shard's bit for bit."""

import math

import numpy as np
import pytest
import torch

from sparkagd_amd import (HostStreamedDenseShard, LogisticGradient,
                          SquaredL2Updater, column_stats, ops, packing, run)
from sparkagd_amd.data import DenseShard
from test_dense_pack import bf16_bits, few_binade_features, ref_encode, ref_table

LOSSES = [ops.LOSS_LOGISTIC, ops.LOSS_LEAST_SQUARES, ops.LOSS_HINGE,
          ops.LOSS_SMOOTH_HINGE]
N, D, CHUNK = 40, 512, 16


def _features(nonfinite=True):
    """Chunk 0 (rows 0-15) without escapes, chunk 1 (16-31) with two,
    chunk 2 (32-39, the partial tail) with three (one, all finite, with
    ``nonfinite=False``: a NaN row would turn every gradient into NaN and
    the comparisons of the evaluation tests into nothing)."""
    x = few_binade_features(N, D, seed=7)
    x[17, 8] = 2.0 ** -30
    x[18, 511] = 2.0 ** 20
    x[34, 3] = -(2.0 ** 20)
    if nonfinite:
        x[33, 250] = float("nan")
        x[39, 0] = float("inf")
    return x.contiguous()


def _vectors():
    g = torch.Generator().manual_seed(11)
    y = (torch.randn(N, generator=g) > 0).float()
    w = torch.randn(D, generator=g) / math.sqrt(D)
    # keeps the margins of the 2^20 rows O(1) (the NaN / inf rows stay so)
    w[511] = 2.0 ** -18
    w[3] = -(2.0 ** -18)
    sw = torch.rand(N, generator=g)
    mask = (torch.rand(N, generator=g) < 0.6).to(torch.uint8)
    return y, w, sw, mask


def _shard(x, y, sw=None, chunk_rows=CHUNK):
    return HostStreamedDenseShard(x.clone(), y, device="cpu",
                                  chunk_rows=chunk_rows, sample_weight=sw)


def _same(a, b):
    """torch.equal with NaNs in the same places counting as equal."""
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and torch.equal(
        a.nan_to_num(1.5, 2.5, 3.5), b.nan_to_num(1.5, 2.5, 3.5)) and \
        torch.equal(torch.isnan(a), torch.isnan(b))


def _all_results(s, w, mask):
    out = []
    for lt in LOSSES:
        out += list(s.eval(w, lt))
        out += list(s.eval(w, lt, need_grad=False))
        out += list(s.eval(w, lt, mask))
    z = s.margins(w)
    out.append(z)
    zf = torch.nan_to_num(z, 0.25, 0.5, -0.5)
    for lt in LOSSES:
        out += list(s.eval_from_margins(zf, lt))
        out += list(s.eval_from_margins(zf, lt, mask))
        out += list(s.eval_from_margins(zf, lt, need_grad=False))
    return out


def _assert_same_results(a, b):
    assert len(a) == len(b)
    for i, (p, q) in enumerate(zip(a, b)):
        assert _same(p, q), f"result {i} differs"


# --- format ------------------------------------------------------------------

def test_packed_bytes_and_side_lists_match_the_resident_pack():
    x = _features()
    y = torch.zeros(N)
    s = _shard(x, y)
    assert s.pack() is True and s.is_packed and s.pack_refused is None
    assert s.pack_seconds is not None and s.pack_seconds >= 0.0
    assert s._pack_table == [0, 59, 60, 61, 62, 63, 64, 65]
    assert s._pack_nnz == 5 and 5 <= packing.PACK_ESCAPE_CAP * N * D
    whole = DenseShard(x.clone(), y)
    assert whole.pack()
    pk = whole._packed
    assert pk.nnz == 5 and pk.table == s._pack_table
    assert s._packed_host.shape == (N, packing.pack_row_bytes(D))
    assert s._packed_host.dtype == torch.uint8
    assert torch.equal(s._packed_host, pk.packed)
    bits = bf16_bits(x)
    ref_packed, _ = ref_encode(bits, ref_table(bits))
    assert np.array_equal(s._packed_host.numpy(), ref_packed)
    # sizes
    assert s.nbytes == N * D * 2
    assert s.streamed_nbytes == N * packing.pack_row_bytes(D)
    # side lists: per chunk, rows local, equal to the whole-shard ones re-based
    assert [nnz for _, nnz in s._pack_esc] == [0, 2, 3]
    rp = pk.esc["rowptr"].long()
    g_rows = torch.repeat_interleave(torch.arange(N), torch.diff(rp))
    c_cols = torch.repeat_interleave(torch.arange(D),
                                     torch.diff(pk.esc["colptr"].long()))
    for i, (lo, hi) in enumerate(s._chunks()):
        esc, nnz = s._pack_esc[i]
        if nnz == 0:
            assert all(v is None for v in esc.values())
            continue
        k0, k1 = int(rp[lo]), int(rp[hi])
        assert k1 - k0 == nnz
        assert all(esc[k].dtype == torch.int32
                   for k in ("rowptr", "col", "colptr", "row"))
        assert torch.equal(esc["rowptr"].long(), rp[lo:hi + 1] - k0)
        assert torch.equal(esc["col"], pk.esc["col"][k0:k1])
        assert torch.equal(esc["val"].view(torch.int32),
                           pk.esc["val"][k0:k1].view(torch.int32))
        assert torch.equal(g_rows[k0:k1], g_rows[k0:k1].clamp(lo, hi - 1))
        in_chunk = (pk.esc["row"] >= lo) & (pk.esc["row"] < hi)
        assert torch.equal(esc["row"], pk.esc["row"][in_chunk] - lo)
        assert torch.equal(esc["cval"].view(torch.int32),
                           pk.esc["cval"][in_chunk].view(torch.int32))
        want_colptr = torch.zeros(D + 1, dtype=torch.int64)
        want_colptr[1:] = torch.cumsum(
            torch.bincount(c_cols[in_chunk], minlength=D), 0)
        assert torch.equal(esc["colptr"].long(), want_colptr)


# --- decoder ---------------------------------------------------------------------

def test_decode_torch_round_trip_keeps_every_bit():
    x = _features()
    x[0, 1] = -0.0
    x[5, 5] = torch.tensor([0x7FC1], dtype=torch.int32).to(torch.int16).view(torch.bfloat16)[0]
    x[33, 250] = torch.tensor([0xFFA5 - 65536], dtype=torch.int16).view(torch.bfloat16)[0]
    pk, why = packing.pack_features(x)
    assert why is None and pk.nnz >= 5
    dec = packing.decode_torch(pk.packed, pk.table, D, pk.esc)
    assert dec.dtype == torch.bfloat16 and dec.shape == x.shape
    assert torch.equal(dec.view(torch.int16), x.view(torch.int16))
    # without the side list the escapes come out as +0.0 and nothing else moves
    bare = packing.decode_torch(pk.packed, pk.table, D, None)
    diff = bare.view(torch.int16) != x.view(torch.int16)
    assert int(diff.sum()) == pk.nnz and (bare.view(torch.int16)[diff] == 0).all()
    # a clean matrix needs no side list
    c = few_binade_features(9, 64, seed=3)
    pc, _ = packing.pack_features(c)
    assert pc.nnz == 0
    assert torch.equal(packing.decode_torch(pc.packed, pc.table, 64, pc.esc)
                       .view(torch.int16), c.view(torch.int16))


# --- evaluation --------------------------------------------------------------------

@pytest.mark.parametrize("release_raw", [False, True])
def test_packed_results_equal_the_unpacked_streamed_shard(release_raw):
    x = _features(nonfinite=False)
    y, w, sw, mask = _vectors()
    raw = _shard(x, y, sw)
    pk = _shard(x, y, sw)
    want_stats = column_stats(raw)
    assert pk.pack(release_raw=release_raw) is True
    assert (pk.features_host is None) == release_raw
    assert pk.feature_dtype == torch.bfloat16
    got, want = _all_results(pk, w, mask), _all_results(raw, w, mask)
    assert all(torch.isfinite(t).all() for t in want if t is not None)
    for i, (p, q) in enumerate(zip(got, want)):
        assert (p is None and q is None) or torch.equal(p, q), f"result {i}"
    # NaN and inf rows propagate exactly as on the raw shard
    raw_nf, pk_nf = _shard(_features(), y, sw), _shard(_features(), y, sw)
    assert pk_nf.pack(release_raw=release_raw)
    z = raw_nf.margins(w)
    assert torch.isnan(z[33]) and torch.isinf(z[39])
    assert _same(pk_nf.margins(w), z)
    got_stats = column_stats(pk)
    for name in ("mean", "variance", "std", "num_nonzeros", "min", "max",
                 "norm_l2"):
        assert _same(getattr(got_stats, name), getattr(want_stats, name)), name
    assert got_stats.count == want_stats.count
    # no packed stream went unused: the CPU route reads the packed bytes
    pk._packed_host.zero_()
    pk._pack_esc = [(packing._no_escapes(), 0)] * len(pk._pack_esc)
    assert float(pk.margins(w).abs().sum()) == 0.0


def test_release_raw_and_unpack_restore_the_features():
    x = _features()
    y, w, sw, mask = _vectors()
    s = _shard(x, y, sw)
    before = _all_results(s, w, mask)
    assert s.pack(release_raw=True) is True
    assert s.features_host is None and s.is_packed
    assert s.nbytes == N * D * 2
    assert s.streamed_nbytes == N * packing.pack_row_bytes(D)
    from sparkagd_amd.models.trainers import _shard_feature_dtype
    from sparkagd_amd.stats import _scale_dtype

    assert _shard_feature_dtype(s) == torch.bfloat16
    assert _scale_dtype(s) == torch.float32
    assert s.pack() is True  # kept
    s.unpack()
    assert not s.is_packed and s.features_host is not None
    assert s.features_host.dtype == torch.bfloat16
    assert torch.equal(s.features_host.view(torch.int16), x.view(torch.int16))
    assert s.streamed_nbytes == s.nbytes
    _assert_same_results(_all_results(s, w, mask), before)
    # releasing later is allowed too
    assert s.pack() and s.features_host is not None
    assert s.pack(release_raw=True) and s.features_host is None


# --- refusals -----------------------------------------------------------------------

def _uniform_bits(n, d):
    g = torch.Generator().manual_seed(0)
    return torch.randint(-32768, 32768, (n, d), generator=g).to(torch.int16) \
        .view(torch.bfloat16)


@pytest.mark.parametrize("make, reason", [
    (lambda: torch.randn(24, 512), "bf16"),
    (lambda: torch.randn(24, 20).to(torch.bfloat16), "multiple of 8"),
    (lambda: few_binade_features(24, 192, seed=2), "not smaller"),
    (lambda: few_binade_features(24, 8, seed=2), "not smaller"),
    (lambda: _uniform_bits(64, 256), "escape fraction"),
], ids=["f32", "d20", "d192", "d8", "uniform-bits"])
def test_refusals_leave_the_shard_streaming_raw(make, reason):
    x = make()
    n, d = x.shape
    g = torch.Generator().manual_seed(1)
    y = (torch.randn(n, generator=g) > 0).float()
    w = (torch.randn(d, generator=g) / math.sqrt(d)).to(
        torch.float32 if x.dtype == torch.bfloat16 else x.dtype)
    s = _shard(x, y, chunk_rows=10)
    before = s.eval(w, ops.LOSS_LOGISTIC)
    for release in (False, True):
        assert s.pack(release_raw=release) is False
        assert not s.is_packed and reason in s.pack_refused
        assert s.features_host is not None
        assert s.streamed_nbytes == s.nbytes
    after = s.eval(w, ops.LOSS_LOGISTIC)
    # (uniform bit patterns hold NaNs: equal where both are NaN)
    assert _same(after[0], before[0]) and _same(after[1], before[1])


# --- cache invalidation ---------------------------------------------------------------

def test_inplace_change_drops_the_packed_copy():
    x = few_binade_features(N, D, seed=9)
    y, w, _, _ = _vectors()
    s = _shard(x, y)
    assert s.pack() and s.is_packed
    first = s._packed_host
    assert s.pack() and s._packed_host is first  # kept, not rebuilt
    s.features_host.neg_()  # any in-place write moves the version counter
    assert not s.is_packed and s._packed_host is None
    assert s.streamed_nbytes == s.nbytes
    fresh = _shard(-x, y)
    assert torch.equal(s.margins(w), fresh.margins(w))
    assert s.pack() and s._packed_host is not first
    assert torch.equal(s.margins(w), fresh.margins(w))
    s.unpack()
    assert not s.is_packed and s.features_host is not None


# --- run() ------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [True, "auto"])
def test_run_leaves_a_cpu_streamed_shard_unpacked(mode):
    x = few_binade_features(N, D, seed=12)
    y, _, _, _ = _vectors()
    s = _shard(x, y)
    w, hist = run(s, LogisticGradient(), SquaredL2Updater(), 0.0,
                  packing.PACK_BREAK_EVEN_ITERS, 1e-3, torch.zeros(D),
                  pack_dense=mode)
    assert not s.is_packed and s.pack_refused is None
    assert len(hist) >= 1 and torch.isfinite(w).all()
