"""Host-streamed bf16 shard streaming its 12-bit packed copy on the GPU: the
packed chunk kernels against the raw-streamed shard (bit-identical without
escapes) and a float64 oracle (with escapes), the HIP decoder against the
input bits, the released-raw mode, back-to-back passes and run()."""

import math

import numpy as np
import pytest
import torch

from sparkagd_amd import (HostStreamedDenseShard, LogisticGradient,
                          SquaredL2Updater, column_stats, ops, packing, run)
from sparkagd_amd.data import DenseShard
from test_dense_pack import bf16_bits, few_binade_features, ref_encode, ref_table
from test_gpu_dense_pack import _escape_features, _vectors

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOSSES = [ops.LOSS_LOGISTIC, ops.LOSS_LEAST_SQUARES, ops.LOSS_HINGE,
          ops.LOSS_SMOOTH_HINGE]
# (37, 1544) / 16: row-group tail, partial wave sweep, 5-row tail chunk;
# (8, 65536) / 3: column slabs, 2-row tail; (4100, 2056) / 1024: several row
# blocks, 4-row tail
CASES = [(37, 1544, 16), (8, 65536, 3), (4100, 2056, 1024)]
IDS = [f"{n}x{d}-chunk{c}" for n, d, c in CASES]


def _streamed(x, y, chunk_rows):
    return HostStreamedDenseShard(x.clone(), y, device=DEV,
                                  chunk_rows=chunk_rows)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


# --- no escapes: bit identity with the raw-streamed shard ----------------------

@pytest.fixture(scope="module", params=CASES, ids=IDS)
def clean_case(request):
    n, d, chunk = request.param
    x = few_binade_features(n, d, seed=n + d)
    y, w, m = _vectors(n, d, seed=d)
    raw = _streamed(x, y, chunk)
    pk = _streamed(x, y, chunk)
    assert pk.pack(), pk.pack_refused
    assert pk.is_packed and pk._pack_nnz == 0
    assert pk.streamed_nbytes == n * packing.pack_row_bytes(d) < pk.nbytes
    return x, y, raw, pk, w


def test_clean_margins_and_eval_equal_raw_streamed(clean_case):
    _, _, raw, pk, w = clean_case
    calls = []
    real = ops.dense_margins_packed

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    ops.dense_margins_packed = spy
    try:
        z_p = pk.margins(w)
    finally:
        ops.dense_margins_packed = real
    assert len(calls) == len(list(pk._chunks())), "not the packed kernels"
    z_r = raw.margins(w)
    assert torch.equal(z_p, z_r)
    mask = (torch.arange(raw.n, device=DEV) % 3 != 0)
    for lt in LOSSES:
        g_r, lc_r = raw.eval(w, lt)
        g_p, lc_p = pk.eval(w, lt)
        assert torch.equal(g_p, g_r) and torch.equal(lc_p, lc_r)
        g_r, lc_r = raw.eval_from_margins(z_r, lt)
        g_p, lc_p = pk.eval_from_margins(z_r, lt)
        assert torch.equal(g_p, g_r) and torch.equal(lc_p, lc_r)
    g_r, lc_r = raw.eval(w, ops.LOSS_LOGISTIC, mask)
    g_p, lc_p = pk.eval(w, ops.LOSS_LOGISTIC, mask)
    assert torch.equal(g_p, g_r) and torch.equal(lc_p, lc_r)
    g_n, lc_n = pk.eval(w, ops.LOSS_LOGISTIC, need_grad=False)
    assert g_n is None
    assert torch.equal(lc_n, raw.eval(w, ops.LOSS_LOGISTIC, need_grad=False)[1])


def test_clean_packed_host_bytes_equal_resident_pack(clean_case):
    x, y, _, pk, _ = clean_case
    res = DenseShard(x.to(DEV), y)
    assert res.pack(), res.pack_refused
    assert res._packed.table == pk._pack_table
    assert pk._packed_host.is_pinned() and not pk._packed_host.is_cuda
    assert torch.equal(pk._packed_host, res._packed.packed.cpu())


def test_non_f32_vector_is_refused_as_on_the_raw_shard(clean_case):
    """A bf16 shard takes f32 vectors, packed or not: the packed shard raises
    the TypeError the raw one does (from the raw route while the raw copy is
    held, from the packed op once it is released)."""
    _, _, raw, pk, w = clean_case
    for s in (raw, pk):
        with pytest.raises(TypeError):
            s.margins(w.double())
        with pytest.raises(TypeError):
            s.eval(w.double(), ops.LOSS_LOGISTIC)


# --- with escapes ------------------------------------------------------------------

@pytest.fixture(scope="module", params=CASES, ids=IDS)
def escape_case(request):
    n, d, chunk = request.param
    x = _escape_features(n, d, seed=n * 3 + d)
    y, w, m = _vectors(n, d, seed=d + 1)
    # the weight damping of test_gpu_dense_pack.escape_case: |z| stays O(1)
    w[d - 1] = 2.0 ** -18
    w[8] = -(2.0 ** -18)
    pk = _streamed(x, y, chunk)
    assert pk.pack(), pk.pack_refused
    assert pk._pack_nnz >= 4
    assert pk._pack_nnz == sum(nnz for _, nnz in pk._pack_esc)
    return x, y, pk, w


def test_escape_counts_and_an_escape_free_chunk():
    """randn at 37 x 1544 leaves about thirty escapes (32 with this seed)
    against a cap of 55; rows 16-31 are made escape-free so that one chunk
    carries no side lists while its neighbours do."""
    n, d, chunk = CASES[0]
    x = _escape_features(n, d, seed=n * 3 + d)
    pk = _streamed(x, torch.zeros(n), chunk)
    assert pk.pack(), pk.pack_refused
    assert int(packing.PACK_ESCAPE_CAP * n * d) == 55 and 4 <= pk._pack_nnz <= 55
    x[16:32] = few_binade_features(16, d, seed=5)[:, :]
    x[16:32] = torch.where(
        torch.isin(((x[16:32].view(torch.int16).int() >> 8) & 0x7F),
                   torch.tensor(pk._pack_table)),
        x[16:32], torch.ones((), dtype=torch.bfloat16))
    y, w, _ = _vectors(n, d, seed=3)
    w[d - 1] = 2.0 ** -18
    w[8] = -(2.0 ** -18)
    s = _streamed(x, y, chunk)
    assert s.pack(), s.pack_refused
    per_chunk = [nnz for _, nnz in s._pack_esc]
    assert per_chunk[1] == 0 and per_chunk[0] > 0 and per_chunk[2] > 0
    assert all(v is None for v in s._pack_esc[1][0].values())
    assert s._pack_esc[0][0]["col"].is_cuda
    z = s.margins(w)
    torch.testing.assert_close(z.double(), x.to(DEV).double() @ w.double(),
                               rtol=2e-4, atol=2e-3)
    g, lc = s.eval(w, ops.LOSS_LOGISTIC)
    g_ref, lc_ref = ops.reference.dense_eval(x.to(DEV).double(), y.double(),
                                             w.double(), ops.LOSS_LOGISTIC)
    torch.testing.assert_close(g.double(), g_ref, rtol=2e-4, atol=2e-3)
    torch.testing.assert_close(lc, lc_ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("loss_type", LOSSES)
def test_escapes_match_f64_oracle(escape_case, loss_type):
    from sparkagd_amd.ops import reference

    x, y, pk, w = escape_case
    xd = x.to(DEV).double()
    g, lc = pk.eval(w, loss_type)
    g_ref, lc_ref = reference.dense_eval(xd, y.double(), w.double(), loss_type)
    torch.testing.assert_close(g.double(), g_ref, rtol=2e-4, atol=2e-3)
    torch.testing.assert_close(lc, lc_ref, rtol=1e-5, atol=1e-6)
    g2, lc2 = pk.eval(w, loss_type)
    assert torch.equal(g2, g) and torch.equal(lc2, lc)  # run to run
    z = pk.margins(w)
    torch.testing.assert_close(z.double(), xd @ w.double(), rtol=2e-4, atol=2e-3)
    assert torch.equal(pk.margins(w), z)
    zf = (xd @ w.double()).float()
    g, lc = pk.eval_from_margins(zf, loss_type)
    g_ref, lc_ref = reference.dense_eval_from_margins(xd, zf.double(),
                                                      y.double(), loss_type)
    torch.testing.assert_close(g.double(), g_ref, rtol=2e-4, atol=2e-3)
    torch.testing.assert_close(lc, lc_ref, rtol=1e-5, atol=1e-6)
    g2, lc2 = pk.eval_from_margins(zf, loss_type)
    assert torch.equal(g2, g) and torch.equal(lc2, lc)


# --- decoder -------------------------------------------------------------------------

def _special_features(n, d, seed):
    x = _escape_features(n, d, seed, special=float("nan"))
    x[3, 9] = float("inf")
    x[4, 10] = float("-inf")
    x[n - 2, d - 8] = -0.0
    x[5, 5] = torch.tensor([0xFFA5 - 65536], dtype=torch.int16).view(torch.bfloat16)[0]
    return x


@pytest.mark.parametrize("n, d, chunk", CASES, ids=IDS)
def test_decoder_restores_every_bit(n, d, chunk):
    x = _special_features(n, d, seed=n + 7)
    s = _streamed(x, torch.zeros(n), chunk)
    assert s.pack(), s.pack_refused
    hip = ops._get_hip()
    for i, (lo, hi) in enumerate(s._chunks()):
        view = s._chunk_view(s._packed_host[lo:hi].to(DEV), i, lo, hi)
        dec = hip.dense_pack_decode(view)
        assert dec.dtype == torch.bfloat16 and dec.shape == (hi - lo, d)
        assert torch.equal(_bits(dec), _bits(x[lo:hi])), f"chunk {i}"
        # into an existing buffer, and the library's torch mirror agrees
        out = torch.full((hi - lo, d), 7.0, dtype=torch.bfloat16, device=DEV)
        assert hip.dense_pack_decode(view, out=out) is out
        assert torch.equal(_bits(out), _bits(x[lo:hi]))
        cpu = packing.decode_torch(view.packed.cpu(), view.table, d,
                                   {k: (None if v is None else v.cpu())
                                    for k, v in view.esc.items()})
        assert torch.equal(_bits(cpu), _bits(x[lo:hi]))


@pytest.mark.parametrize("n, d, chunk", CASES, ids=IDS)
def test_release_raw_column_stats_and_unpack(n, d, chunk):
    x = _escape_features(n, d, seed=n + 11)
    x[n - 2, d - 8] = -0.0
    y, w, _ = _vectors(n, d, seed=d + 2)
    w[d - 1] = 2.0 ** -18
    w[8] = -(2.0 ** -18)
    held = _streamed(x, y, chunk)
    assert held.pack(), held.pack_refused
    s = _streamed(x, y, chunk)
    assert s.pack(release_raw=True), s.pack_refused
    assert s.features_host is None and s.is_packed
    assert s.feature_dtype == torch.bfloat16 and s.nbytes == n * d * 2
    assert s.streamed_nbytes == n * packing.pack_row_bytes(d)
    # the packed passes do not depend on the raw copy
    assert torch.equal(s.margins(w), held.margins(w))
    g_s, lc_s = s.eval(w, ops.LOSS_LOGISTIC)
    g_h, lc_h = held.eval(w, ops.LOSS_LOGISTIC)
    assert torch.equal(g_s, g_h) and torch.equal(lc_s, lc_h)
    with pytest.raises(TypeError):
        s.margins(w.double())
    # a raw-chunk consumer gets decoded chunks. Same chunks, same bits: the
    # summary of the raw-streamed shard, exactly
    got = column_stats(s)
    same_chunks = column_stats(_streamed(x, y, chunk))
    for name in ("mean", "variance", "std", "num_nonzeros", "min", "max",
                 "norm_l2"):
        assert torch.equal(getattr(got, name), getattr(same_chunks, name)), name
    # and the resident shard's: exactly where the order of summation cannot
    # matter, and within test_streamed_shard_stats_gpu's bounds for the f64
    # sums that the chunk loop adds up in another order than one pass does
    want = column_stats(DenseShard(x.to(DEV), y))
    assert got.count == want.count == n
    for name in ("num_nonzeros", "min", "max"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    xd = x.to(DEV).double()
    sabs, sq = xd.abs().sum(0), (xd * xd).sum(0)
    assert ((got.mean - want.mean).abs() * n <= 1e-9 * sabs + 1e-300).all()
    assert ((got.variance - want.variance).abs() <= 1e-9 * (sq / n)).all()
    torch.testing.assert_close(got.norm_l2, want.norm_l2, rtol=1e-9, atol=0.0)
    s.unpack()
    assert not s.is_packed and s.streamed_nbytes == s.nbytes
    assert s.features_host.is_pinned() and s.features_host.dtype == torch.bfloat16
    assert torch.equal(_bits(s.features_host), _bits(x))
    raw = _streamed(x, y, chunk)
    assert torch.equal(s.margins(w), raw.margins(w))


# --- back-to-back passes ----------------------------------------------------------------

def test_packed_back_to_back_passes_no_corruption():
    """Packed twin of test_streamed_back_to_back_passes_no_corruption: two
    feature passes with no host synchronise between them must not let the
    second pass's H2D copies overwrite packed chunks that the first pass's
    tail kernels still read."""
    g = torch.Generator().manual_seed(41)
    n, d = 16384, 2048
    feats = torch.randn((n, d), generator=g).to(torch.bfloat16)
    labels = (torch.rand(n, generator=g) < 0.5).float()
    res = DenseShard(feats.to(DEV), labels.to(DEV))
    assert res.pack(), res.pack_refused
    st = HostStreamedDenseShard(feats, labels, device=DEV, chunk_rows=1024)
    assert st.pack(), st.pack_refused
    x = torch.randn(d, generator=g).to(DEV)
    z = torch.randn(d, generator=g).to(DEV)
    ref_x = res.margins(x)
    ref_z = res.margins(z)
    for _ in range(3):
        mx = st.margins(x)   # no torch.cuda.synchronize between these
        mz = st.margins(z)
        torch.testing.assert_close(mx, ref_x, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(mz, ref_z, rtol=1e-4, atol=1e-4)


# --- run() ----------------------------------------------------------------------------------

def test_run_pack_dense_on_a_streamed_shard():
    n, d, chunk = 512, 4096, 128
    x = few_binade_features(n, d, seed=21)
    g = torch.Generator().manual_seed(23)
    w_true = torch.randn(d, generator=g) / math.sqrt(d)
    y = (x.float() @ w_true > 0).float()
    w0 = torch.zeros(d, device=DEV)
    out = {}
    for mode in (False, True, "auto"):
        s = _streamed(x, y, chunk)
        out[mode] = run(s, LogisticGradient(), SquaredL2Updater(), 0.0,
                        packing.PACK_BREAK_EVEN_ITERS if mode == "auto" else 12,
                        1e-3, w0, 1.0, math.inf, 0.5, 0.9, True,
                        pack_dense=mode)
        assert s.is_packed == (mode is True), (mode, s.pack_refused)
    (w_r, h_r), (w_p, h_p) = out[False], out[True]
    assert len(h_r) == len(h_p) == 12
    assert h_p == h_r and torch.equal(w_p, w_r)


def test_multiclass_gradient_packs_no_streamed_shard():
    from sparkagd_amd import MultinomialLogisticGradient

    n, d = 64, 512
    s = _streamed(few_binade_features(n, d, seed=4), torch.zeros(n), 16)
    packing.apply_pack_policy(s, True, 100, MultinomialLogisticGradient(3))
    assert not s.is_packed
    packing.apply_pack_policy(s, "auto", 100, LogisticGradient())
    assert not s.is_packed
    packing.apply_pack_policy(s, True, 100, LogisticGradient())
    assert s.is_packed
