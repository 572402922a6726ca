"""12-bit packed bf16 shard: format, table choice and pack policy (CPU).

The encoder/decoder below are an independent numpy statement of the format
in docs/KERNELS.md ("Packed bf16 stream"); the GPU tests compare the device
encoder against them byte for byte.
"""

import numpy as np
import pytest
import torch

from sparkagd_amd import packing
from sparkagd_amd.config import AGDConfig
from sparkagd_amd.data import DenseShard, InterceptShard


# --- reference encoder / decoder -------------------------------------------

def bf16_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.uint16)


def ref_table(bits: np.ndarray):
    hist = np.bincount(((bits >> 8) & 0x7F).reshape(-1), minlength=128)
    return packing.choose_pack_table(hist.tolist())[0]


def ref_encode(bits: np.ndarray, table):
    """bits [n, d] uint16 -> (packed [n, row bytes] uint8, escape mask [n, d]).
    Rows are padded with zero groups to a multiple of 32 groups (384 B)."""
    n, d = bits.shape
    assert d % 8 == 0 and table[0] == 0
    gs = -(-(d // 8) // 32) * 32
    out = np.zeros((n, gs, 12), dtype=np.uint8)
    esc = np.zeros((n, d), dtype=bool)
    for r in range(n):
        for g in range(d // 8):
            for k in range(8):
                u = int(bits[r, g * 8 + k])
                h = (u >> 8) & 0x7F
                if h not in table:
                    esc[r, g * 8 + k] = True  # stored as +0.0: all-zero code
                    continue
                code = ((u >> 15) << 3) | table.index(h)
                out[r, g, k] = u & 0xFF
                out[r, g, 8 + (k & 3)] |= code << (4 * (k >> 2))
    return out.reshape(n, gs * 12), esc


def ref_decode(packed: np.ndarray, table, d: int) -> np.ndarray:
    """packed bytes -> bf16 bit patterns [n, d] (escapes come out as 0)."""
    n = packed.shape[0]
    p = packed.reshape(n, -1, 12)[:, :d // 8]
    bits = np.zeros((n, d), dtype=np.uint16)
    for k in range(8):
        code = (p[:, :, 8 + (k & 3)] >> (4 * (k >> 2))) & 0xF
        hi = np.asarray(table, dtype=np.uint16)[code & 7] | ((code >> 3) << 7)
        bits[:, k::8] = (hi << 8) | p[:, :, k]
    return bits


def bits_to_bf16(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(bits.astype(np.int16)).view(torch.bfloat16)


def few_binade_features(n, d, seed, with_zero=True):
    """bf16 values from at most 8 high-byte magnitudes, both signs, +-0."""
    g = torch.Generator().manual_seed(seed)
    highs = torch.tensor([0x00, 0x3B, 0x3C, 0x3D, 0x3E, 0x3F, 0x40, 0x41])
    h = highs[torch.randint(0, 8, (n, d), generator=g)]
    low = torch.randint(0, 256, (n, d), generator=g)
    sign = torch.randint(0, 2, (n, d), generator=g)
    bits = (sign << 15) | (h << 8) | low
    if with_zero:
        bits[0, 0] = 0x0000
        bits[0, 1] = 0x8000
    # high byte 0x00 with a nonzero low byte is a subnormal/tiny value: keep
    # a few, zero the rest so the data stays well scaled
    tiny = (h == 0)
    bits = torch.where(tiny & (low > 3), (sign << 15), bits)
    return bits.to(torch.int32).to(torch.int16).view(torch.bfloat16).contiguous()


# --- table choice -----------------------------------------------------------

def test_table_is_top8_sorted_with_zero_slot():
    hist = [0] * 128
    for v, c in [(63, 900), (62, 800), (61, 700), (64, 600), (60, 500),
                 (59, 400), (58, 300), (57, 200), (56, 100), (0, 50)]:
        hist[v] = c
    table, esc = packing.choose_pack_table(hist)
    # 0x00 is not in the top 8: it replaces the least frequent of them
    assert table == [0, 58, 59, 60, 61, 62, 63, 64]
    assert esc == 200 + 100
    lo, hi = packing.table_luts(table)
    assert lo & 0xFF == 0
    assert [(lo >> (8 * i)) & 0xFF for i in range(4)] + \
           [(hi >> (8 * i)) & 0xFF for i in range(4)] == table


def test_table_keeps_zero_when_frequent():
    hist = [0] * 128
    hist[0] = 10_000
    for v in range(60, 67):
        hist[v] = 100 + v
    table, esc = packing.choose_pack_table(hist)
    assert table == [0, 60, 61, 62, 63, 64, 65, 66] and esc == 0


def test_table_choice_deterministic_under_ties():
    hist = [0] * 128
    for v in range(50, 70):
        hist[v] = 1000  # 20-way tie
    hist[0] = 1000
    t1, _ = packing.choose_pack_table(hist)
    t2, _ = packing.choose_pack_table(list(hist))
    # ties go to the lower value: 0 and 50..56
    assert t1 == t2 == [0, 50, 51, 52, 53, 54, 55, 56]
    # an all-zero histogram still yields a valid table
    assert packing.choose_pack_table([0] * 128)[0] == list(range(8))


# --- round trip ---------------------------------------------------------------

@pytest.mark.parametrize("kind", ["few", "randn"])
def test_encode_decode_round_trip_cpu(kind, monkeypatch):
    # the cap is policy, not format: 1024 elements admit a single escape
    monkeypatch.setattr(packing, "PACK_ESCAPE_CAP", 1.0)
    n, d = 16, 64
    if kind == "few":
        x = few_binade_features(n, d, seed=3)
    else:
        x = torch.randn(n, d, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16)
        x[1, 5] = 2.0 ** -30
        x[2, 9] = 2.0 ** 20
        x[3, 0] = float("inf")
        x[4, 63] = float("nan")
    bits = bf16_bits(x)
    table = ref_table(bits)
    packed, esc = ref_encode(bits, table)
    # the library's torch encoder writes the same bytes
    pk, why = packing.pack_features(x)
    assert why is None and pk.table == table
    assert np.array_equal(pk.packed.numpy(), packed)
    assert pk.nnz == int(esc.sum())
    # decoded values + escapes reproduce the input bit for bit
    dec = ref_decode(packed, table, d)
    assert np.array_equal(dec[~esc], bits[~esc])
    assert np.all(dec[esc] == 0)
    if pk.nnz:
        rp = pk.esc["rowptr"].numpy()
        rows = np.repeat(np.arange(n), np.diff(rp))
        cols = pk.esc["col"].numpy()
        assert np.array_equal(np.argwhere(esc), np.stack([rows, cols], 1))
        want = x.float()[torch.from_numpy(esc)]
        got = pk.esc["val"]
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        # column-sorted copy holds the same entries
        cp = pk.esc["colptr"].numpy()
        ccols = np.repeat(np.arange(d), np.diff(cp))
        crow = pk.esc["row"].numpy()
        assert sorted(zip(rows.tolist(), cols.tolist())) == \
            sorted(zip(crow.tolist(), ccols.tolist()))
        assert np.all(np.diff(ccols) >= 0)
    if kind == "few":
        assert pk.nnz == 0


# --- policy --------------------------------------------------------------------

def _shard(x):
    return DenseShard(x, torch.zeros(x.shape[0]))


def test_pack_refuses_d_not_multiple_of_8():
    s = _shard(torch.randn(5, 12).to(torch.bfloat16))
    assert s.pack() is False and not s.is_packed
    assert "multiple of 8" in s.pack_refused


def test_pack_refuses_non_bf16():
    s = _shard(torch.randn(5, 16))
    assert s.pack() is False and "bf16" in s.pack_refused


def test_pack_refuses_uniform_bit_patterns():
    g = torch.Generator().manual_seed(0)
    bits = torch.randint(-32768, 32768, (64, 256), generator=g).to(torch.int16)
    s = _shard(bits.view(torch.bfloat16))
    assert s.pack() is False and not s.is_packed
    assert "escape fraction" in s.pack_refused


def test_inplace_change_drops_the_cache():
    s = _shard(few_binade_features(8, 64, seed=1))
    assert s.pack() and s.is_packed
    first = s._packed
    assert s.pack() and s._packed is first  # kept, not rebuilt
    s.features.neg_()  # any in-place write moves the version counter
    assert not s.is_packed
    assert s.pack() and s._packed is not first
    s.unpack()
    assert not s.is_packed
    # a wrapped shard packs through its inner shard
    w = InterceptShard(s)
    packing.apply_pack_policy(w, "auto", 100)  # CPU: auto never packs
    assert not s.is_packed


def test_gradient_streams_shard():
    from sparkagd_amd import (LogisticGradient, MultinomialLogisticGradient,
                              HingeGradient)

    class Wrapper:  # what bench.py's counting wrapper looks like
        def __init__(self, inner):
            self.inner = inner

    class OwnKernels(LogisticGradient):
        def margins(self, shard, v):
            return shard.features.float() @ v

    assert packing.gradient_streams_shard(LogisticGradient())
    assert packing.gradient_streams_shard(Wrapper(Wrapper(HingeGradient())))
    assert not packing.gradient_streams_shard(MultinomialLogisticGradient(3))
    assert not packing.gradient_streams_shard(Wrapper(MultinomialLogisticGradient(3)))
    assert not packing.gradient_streams_shard(OwnKernels())
    assert not packing.gradient_streams_shard(object())


def test_nbytes_reports_the_raw_shard():
    s = _shard(few_binade_features(8, 64, seed=2))
    before = s.nbytes
    assert s.pack()
    assert s.nbytes == before


def test_policy_false_and_auto_gates(monkeypatch):
    s = _shard(few_binade_features(8, 64, seed=5))
    packing.apply_pack_policy(s, False, 1000)
    assert not s.is_packed
    # auto: CPU tensors, short runs and cache-sized shards are not packed
    assert not packing.auto_pack_wanted(s.features, 1000)
    AGDConfig(pack_dense=False).validate()
    AGDConfig(pack_dense=True).validate()
    with pytest.raises(ValueError):
        AGDConfig(pack_dense="yes").validate()
    assert AGDConfig().pack_dense == "auto"
