"""12-bit packed bf16 shard on the GPU: the packed stream kernels against the
raw bf16 path (bit-identical without escapes), against a float64 oracle
(with escapes), the device encoder against the CPU reference, and run()."""

import math

import numpy as np
import pytest
import torch

from sparkagd_amd import LogisticGradient, SquaredL2Updater, ops, run
from sparkagd_amd.data import DenseShard, InterceptShard
from conftest import assert_rel
from test_dense_pack import (bf16_bits, few_binade_features, ref_decode,
                             ref_encode, ref_table)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOSSES = [ops.LOSS_LOGISTIC, ops.LOSS_LEAST_SQUARES, ops.LOSS_HINGE,
          ops.LOSS_SMOOTH_HINGE]
# (37, 1544): row-group tail + partial wave sweep; (8, 65536): column slabs
# (n_slabs > 1); (4100, 2056): several row blocks + a partial column block
SHAPES = [(37, 1544), (8, 65536), (4100, 2056)]


def _vectors(n, d, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    y = (torch.randn(n, generator=g, device=DEV) > 0).to(torch.float32)
    w = torch.randn(d, generator=g, device=DEV) / math.sqrt(d)
    m = torch.randn(n, generator=g, device=DEV)
    return y, w, m


def _pair(x, y):
    raw = DenseShard(x.to(DEV), y)
    pk = DenseShard(x.to(DEV).clone(), y)
    assert pk.pack(), pk.pack_refused
    return raw, pk


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def clean_case(request):
    n, d = request.param
    x = few_binade_features(n, d, seed=n + d)
    y, w, m = _vectors(n, d, seed=d)
    raw, pk = _pair(x, y)
    assert pk._packed.nnz == 0
    return raw, pk, w, m


def test_bit_identity_margins(clean_case):
    raw, pk, w, _ = clean_case
    assert torch.equal(pk.margins(w), raw.margins(w))


@pytest.mark.parametrize("loss_type", LOSSES)
def test_bit_identity_eval_from_margins(clean_case, loss_type):
    raw, pk, w, _ = clean_case
    z = raw.margins(w)
    g_r, lc_r = raw.eval_from_margins(z, loss_type)
    g_p, lc_p = pk.eval_from_margins(z, loss_type)
    assert torch.equal(g_p, g_r) and torch.equal(lc_p, lc_r)
    # the fused evaluation (margins + multiplier + gradient) as well
    g_r2, lc_r2 = raw.eval(w, loss_type)
    g_p2, lc_p2 = pk.eval(w, loss_type)
    assert torch.equal(g_p2, g_r2) and torch.equal(lc_p2, lc_r2)


def test_bit_identity_grad_from_mult_with_zero_rows(clean_case):
    raw, pk, _, m = clean_case
    assert torch.equal(pk.grad_from_mult(m), raw.grad_from_mult(m))
    mz = m.clone()
    mz[::3] = 0.0   # breaks the 4-row groups of the unrolled sweep
    mz[-5:] = 0.0
    assert torch.equal(pk.grad_from_mult(mz), raw.grad_from_mult(mz))
    assert torch.equal(pk.grad_from_mult(torch.zeros_like(m)),
                       torch.zeros(raw.d, device=DEV))


def test_bit_identity_intercept_and_mask(clean_case):
    raw, pk, w, _ = clean_case
    wb = torch.cat([w, torch.tensor([0.25], device=DEV)])
    g_r, lc_r = InterceptShard(raw).eval(wb, ops.LOSS_LOGISTIC)
    g_p, lc_p = InterceptShard(pk).eval(wb, ops.LOSS_LOGISTIC)
    assert torch.equal(g_p, g_r) and torch.equal(lc_p, lc_r)
    mask = (torch.arange(raw.n, device=DEV) % 2 == 0)
    g_r, lc_r = raw.eval(w, ops.LOSS_LOGISTIC, mask)
    g_p, lc_p = pk.eval(w, ops.LOSS_LOGISTIC, mask)
    assert torch.equal(g_p, g_r) and torch.equal(lc_p, lc_r)


# --- with escapes ------------------------------------------------------------

def _escape_features(n, d, seed, special=None):
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16)
    x[0, 0] = 2.0 ** -30
    x[n // 2, d // 2] = 2.0 ** -30
    x[n - 1, d - 1] = 2.0 ** 20
    x[1, 8] = -(2.0 ** 20)
    if special is not None:
        x[2, 17] = special
    return x.contiguous()


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def escape_case(request):
    n, d = request.param
    x = _escape_features(n, d, seed=n * 3 + d)
    y, w, m = _vectors(n, d, seed=d + 1)
    # f32 margins carry an error of ulp(|z|): with w ~ d^-1/2 a 2^20 feature
    # would push |z| to ~10^4 and that ulp alone past the gradient tolerance.
    # 2^-18 at the two planted columns keeps |z| = O(1) while each escape
    # still moves its margin by 4, two thousand times the tolerance.
    w[d - 1] = 2.0 ** -18
    w[8] = -(2.0 ** -18)
    raw, pk = _pair(x, y)
    assert pk._packed.nnz >= 4
    return x, raw, pk, y, w, m


def test_escapes_margins_match_f64_oracle(escape_case):
    x, _, pk, _, w, _ = escape_case
    z = pk.margins(w)
    ref = x.to(DEV).double() @ w.double()
    torch.testing.assert_close(z.double(), ref, rtol=2e-4, atol=2e-3)
    assert torch.equal(pk.margins(w), z)  # run to run


@pytest.mark.parametrize("loss_type", LOSSES)
def test_escapes_eval_matches_f64_oracle(escape_case, loss_type):
    from sparkagd_amd.ops import reference

    x, _, pk, y, w, _ = escape_case
    g, lc = pk.eval(w, loss_type)
    g_ref, lc_ref = reference.dense_eval(x.to(DEV).double(), y.double(),
                                         w.double(), loss_type)
    torch.testing.assert_close(g.double(), g_ref, rtol=2e-4, atol=2e-3)
    torch.testing.assert_close(lc, lc_ref, rtol=1e-5, atol=1e-6)
    g2, lc2 = pk.eval(w, loss_type)
    assert torch.equal(g2, g) and torch.equal(lc2, lc)


@pytest.mark.parametrize("loss_type", LOSSES)
def test_escapes_eval_from_margins_matches_f64_oracle(escape_case, loss_type):
    """Mode 2 (margins given) on a shard with escapes: multiplier, then the
    packed gradient stream plus the column-sorted correction."""
    from sparkagd_amd.ops import reference

    x, _, pk, y, w, _ = escape_case
    z = (x.to(DEV).double() @ w.double()).float()
    g, lc = pk.eval_from_margins(z, loss_type)
    g_ref, lc_ref = reference.dense_eval_from_margins(
        x.to(DEV).double(), z.double(), y.double(), loss_type)
    torch.testing.assert_close(g.double(), g_ref, rtol=2e-4, atol=2e-3)
    torch.testing.assert_close(lc, lc_ref, rtol=1e-5, atol=1e-6)
    g2, lc2 = pk.eval_from_margins(z, loss_type)
    assert torch.equal(g2, g) and torch.equal(lc2, lc)


def test_escapes_intercept_shard(escape_case):
    """InterceptShard over a packed inner shard with escapes, against the
    same wrapper over the raw shard."""
    _, raw, pk, _, w, _ = escape_case
    wb = torch.cat([w, torch.tensor([-0.5], device=DEV)])
    g_r, lc_r = InterceptShard(raw).eval(wb, ops.LOSS_LOGISTIC)
    g_p, lc_p = InterceptShard(pk).eval(wb, ops.LOSS_LOGISTIC)
    torch.testing.assert_close(g_p, g_r, rtol=2e-4, atol=2e-3)
    torch.testing.assert_close(lc_p, lc_r, rtol=1e-5, atol=1e-6)


def test_mixed_shard_dense_part_takes_the_packed_route():
    """apply_pack_policy reaches the dense part of a MixedShard (also under
    an InterceptShard) and the packed part computes what the raw one does."""
    from sparkagd_amd import packing
    from sparkagd_amd.data import MixedShard, generate_csr_problem

    n, d = 300, 1544
    y, w, _ = _vectors(n, d, seed=17)
    x = few_binade_features(n, d, seed=18).to(DEV)
    csr, _ = generate_csr_problem(200, d, 8, seed=19, device=DEV)
    raw = MixedShard([DenseShard(x, y), csr])
    dense_pk = DenseShard(x.clone(), y)
    mixed = MixedShard([dense_pk, csr])
    packing.apply_pack_policy(InterceptShard(mixed), True, 1, LogisticGradient())
    assert dense_pk.is_packed
    calls = []
    real = ops.dense_eval_packed

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    ops.dense_eval_packed = spy
    try:
        g_p, lc_p = mixed.eval(w, ops.LOSS_LOGISTIC)
    finally:
        ops.dense_eval_packed = real
    assert calls, "the dense part did not go through the packed kernels"
    g_r, lc_r = raw.eval(w, ops.LOSS_LOGISTIC)
    assert torch.equal(g_p, g_r) and torch.equal(lc_p, lc_r)
    assert torch.equal(mixed.margins(w), raw.margins(w))


def test_escapes_grad_from_mult_matches_f64_oracle(escape_case):
    x, _, pk, _, _, m = escape_case
    g = pk.grad_from_mult(m)
    ref = x.to(DEV).double().t() @ m.double()
    # 2^20 entries make the column sums large: the bound is relative to them
    torch.testing.assert_close(g.double(), ref, rtol=2e-4, atol=2e-3)
    assert torch.equal(pk.grad_from_mult(m), g)


@pytest.mark.parametrize("special", [float("inf"), float("nan")])
def test_nonfinite_propagates_as_on_raw_path(special):
    n, d = 37, 1544
    x = _escape_features(n, d, seed=99, special=special)
    y, w, m = _vectors(n, d, seed=5)
    raw, pk = _pair(x, y)
    z_r, z_p = raw.margins(w), pk.margins(w)
    assert torch.equal(torch.isnan(z_p), torch.isnan(z_r))
    assert torch.equal(torch.isinf(z_p), torch.isinf(z_r))
    fin = torch.isfinite(z_r)
    assert torch.equal(z_p[~fin].nan_to_num(1.0, 2.0, 3.0),
                       z_r[~fin].nan_to_num(1.0, 2.0, 3.0))
    torch.testing.assert_close(z_p[fin], z_r[fin], rtol=2e-4, atol=2e-3)
    for mult in (m, torch.where(torch.arange(n, device=DEV) == 2,
                                torch.zeros_like(m), m)):
        g_r, g_p = raw.grad_from_mult(mult), pk.grad_from_mult(mult)
        assert torch.equal(torch.isnan(g_p), torch.isnan(g_r))
        assert torch.equal(torch.isinf(g_p), torch.isinf(g_r))
        fin = torch.isfinite(g_r)
        torch.testing.assert_close(g_p[fin], g_r[fin], rtol=2e-4, atol=2e-3)
    # the row with the non-finite feature skipped (m == 0): all finite
    assert torch.isfinite(g_p).all()


# --- encoder round trip --------------------------------------------------------

@pytest.mark.parametrize("kind", ["few", "randn"])
def test_gpu_packed_bytes_equal_cpu_reference(kind, monkeypatch):
    from sparkagd_amd import packing

    # the cap is policy, not format: 1024 elements admit a single escape
    monkeypatch.setattr(packing, "PACK_ESCAPE_CAP", 1.0)
    n, d = 16, 64
    if kind == "few":
        x = few_binade_features(n, d, seed=3)
    else:
        x = _escape_features(n, d, seed=4, special=float("inf"))
    bits = bf16_bits(x)
    table = ref_table(bits)
    packed_ref, esc = ref_encode(bits, table)
    s = DenseShard(x.to(DEV), torch.zeros(n, device=DEV))
    assert s.pack(), s.pack_refused
    pk = s._packed
    assert pk.table == table
    assert np.array_equal(pk.packed.cpu().numpy(), packed_ref)
    dec = ref_decode(pk.packed.cpu().numpy(), table, d)
    assert np.array_equal(dec[~esc], bits[~esc])
    assert pk.nnz == int(esc.sum())
    if pk.nnz:
        rows = np.repeat(np.arange(n), np.diff(pk.esc["rowptr"].cpu().numpy()))
        cols = pk.esc["col"].cpu().numpy()
        assert np.array_equal(np.argwhere(esc), np.stack([rows, cols], 1))
        want = x.float()[torch.from_numpy(esc)]
        assert torch.equal(pk.esc["val"].cpu().view(torch.int32),
                           want.view(torch.int32))
        ccols = np.repeat(np.arange(d), np.diff(pk.esc["colptr"].cpu().numpy()))
        crow = pk.esc["row"].cpu().numpy()
        assert list(zip(ccols.tolist(), crow.tolist())) == \
            sorted(zip(cols.tolist(), rows.tolist()))
        assert torch.equal(pk.esc["cval"].cpu().view(torch.int32),
                           x.float()[crow, ccols].view(torch.int32))


# --- policy on the device --------------------------------------------------------

def test_policy_on_device(monkeypatch):
    from sparkagd_amd import StandardScaler, packing

    n, d = 64, 256
    y, w, _ = _vectors(n, d, seed=1)
    s = DenseShard(few_binade_features(n, d, seed=8).to(DEV), y)
    iters = packing.PACK_BREAK_EVEN_ITERS
    args = (LogisticGradient(), SquaredL2Updater(), 0.0, iters, 1e-3,
            torch.zeros(d, device=DEV), 1.0, math.inf, 0.5, 0.9, True)
    run(s, *args, pack_dense=False)
    assert not s.is_packed
    run(s, *args)  # auto: far below the Infinity Cache size
    assert not s.is_packed
    monkeypatch.setattr(packing, "PACK_MIN_BYTES", 0)
    monkeypatch.setattr(packing, "PACK_HEADROOM_BYTES", 0)
    run(s, *args[:3], iters - 1, *args[4:])  # one short of the break-even
    assert not s.is_packed
    run(s, *args)
    assert s.is_packed
    # in-place standardisation invalidates the copy
    StandardScaler().fit(s).transform(s, inplace=True)
    assert not s.is_packed
    s2 = DenseShard(few_binade_features(n, d, seed=9).to(DEV), y)
    run(s2, *args[:3], 2, *args[4:], pack_dense=True)  # True: no gates
    assert s2.is_packed
    # d % 8 != 0 and a too-wide exponent spread stay on the raw path
    odd = DenseShard(torch.randn(n, 252, device=DEV).to(torch.bfloat16), y)
    run(odd, LogisticGradient(), SquaredL2Updater(), 0.0, 8, 1e-3,
        torch.zeros(252, device=DEV), pack_dense=True)
    assert not odd.is_packed and "multiple of 8" in odd.pack_refused
    bits = torch.randint(-32768, 32768, (n, d), device=DEV).to(torch.int16)
    wide = DenseShard(bits.view(torch.bfloat16), y)
    assert wide.pack() is False and "escape fraction" in wide.pack_refused
    # a features tensor swapped for a strided view is refused, not asserted on
    s2.unpack()
    s2.features = torch.empty(n, 2 * d, device=DEV, dtype=torch.bfloat16)[:, :d]
    assert s2.pack() is False and "contiguous" in s2.pack_refused
    # the environment replaces the "auto" default only
    monkeypatch.setenv("SPARKAGD_PACK_DENSE", "1")
    s3 = DenseShard(few_binade_features(n, d, seed=10).to(DEV), y)
    run(s3, *args[:3], 2, *args[4:], pack_dense=False)
    assert not s3.is_packed
    run(s3, *args[:3], 2, *args[4:])
    assert s3.is_packed


def test_multiclass_run_never_packs(monkeypatch):
    """The multiclass gradient streams shard.features through its own
    kernels: a packed copy would only cost memory, under auto and True."""
    from sparkagd_amd import MultinomialLogisticGradient, packing
    from sparkagd_amd.data import generate_multiclass_problem

    monkeypatch.setattr(packing, "PACK_MIN_BYTES", 0)
    monkeypatch.setattr(packing, "PACK_HEADROOM_BYTES", 0)
    k, d = 3, 256
    shard, _ = generate_multiclass_problem(512, d, k, seed=3, device=DEV,
                                           dtype=torch.bfloat16)
    w0 = torch.zeros(d * k, device=DEV)
    for mode, iters in (("auto", packing.PACK_BREAK_EVEN_ITERS), (True, 2)):
        run(shard, MultinomialLogisticGradient(k), SquaredL2Updater(), 0.0,
            iters, 1e-3, w0, pack_dense=mode)
        assert not shard.is_packed


# --- trajectory -------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["few", "randn"])
def test_trajectory_packed_vs_raw(kind):
    n, d = 512, 4096
    if kind == "few":
        x = few_binade_features(n, d, seed=21)
    else:
        x = _escape_features(n, d, seed=22)
    g = torch.Generator().manual_seed(23)
    w_true = torch.randn(d, generator=g) / math.sqrt(d)
    y = (x.float() @ w_true > 0).float().to(DEV)
    w0 = torch.zeros(d, device=DEV)
    out = {}
    for pack in (False, True):
        s = DenseShard(x.to(DEV).clone(), y)
        out[pack] = run(s, LogisticGradient(), SquaredL2Updater(), 0.0, 20,
                        1e-3, w0, 1.0, math.inf, 0.5, 0.9, True,
                        pack_dense=pack)
        assert s.is_packed == pack
    (w_r, h_r), (w_p, h_p) = out[False], out[True]
    assert len(h_r) == len(h_p) == 20
    if kind == "few":
        assert h_p == h_r and torch.equal(w_p, w_r)
    else:
        for a, b in zip(h_r, h_p):
            assert_rel(a, b, 1e-3, "packed vs raw loss history")
        torch.testing.assert_close(w_p, w_r, rtol=5e-3, atol=5e-3)
