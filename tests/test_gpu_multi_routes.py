"""``multi_margins`` / ``multi_grad`` reach the kernel that the routing table
names (bit for bit the direct call), and the softmax and the multi-task
gradient classes share that route.

Shapes: n = 80 is a ragged third 32-row block, d = 272 one 16-byte unit past
a 256-column step, k = 3 is KC 4 in one class tile, k = 33 is KC 36 across
the 32-column template boundary (CSR: k = 40, a 32-column chunk plus one of
8)."""

import pytest
import torch

from sparkagd_amd import (
    DenseShard, LogisticGradient, MultinomialLogisticGradient,
    MultiTaskGradient, ops, packing,
)
from sparkagd_amd.data import generate_multiclass_csr_problem
from sparkagd_amd.ops import hiplib
from sparkagd_amd.ops import multiclass as mc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, D = 80, 272
F8 = torch.float8_e4m3fn


def _dense(dtype, pack=False):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, D, generator=g).to(dtype)
    shard = DenseShard(x.to(DEV), torch.zeros(N, device=DEV))
    if pack:
        assert shard.pack(), shard.pack_refused
    return shard


def _csr():
    shard, _ = generate_multiclass_csr_problem(N, D, 8, num_classes=3, seed=13,
                                               device=DEV)
    return shard


def _w_m(k):
    """(W flat [d*k], padded M flat [n*KC] with exact-zero pad columns)."""
    g = torch.Generator().manual_seed(k)
    kc = mc.padded_k(k)
    w = torch.randn(D * k, generator=g) / D ** 0.5
    m = torch.zeros(N, kc)
    m[:, :k] = torch.randn(N, k, generator=g)
    return w.to(DEV), m.reshape(-1).to(DEV)


def _unpad(gradp, k):
    return gradp.reshape(D, mc.padded_k(k))[:, :k].reshape(-1).contiguous()


def _clear_env(monkeypatch):
    monkeypatch.delenv("SPARKAGD_MULTI_MARGINS", raising=False)
    monkeypatch.delenv("SPARKAGD_MULTI_GRAD", raising=False)


def _set_env(monkeypatch, algo):
    monkeypatch.setenv("SPARKAGD_MULTI_MARGINS", algo)
    monkeypatch.setenv("SPARKAGD_MULTI_GRAD", algo)


# --- each route is the direct call the table names ---

@pytest.mark.parametrize("k", [3, 33])
def test_bf16_takes_the_gemms(k, monkeypatch):
    _clear_env(monkeypatch)
    shard, (w, m) = _dense(torch.bfloat16), _w_m(k)
    a, kc = shard.features, mc.padded_k(k)
    wt = torch.zeros((kc, D), dtype=torch.bfloat16, device=DEV)
    wt[:k] = w.reshape(D, k).T.to(torch.bfloat16)
    z = torch.empty((N, kc), dtype=torch.float32, device=DEV)
    hiplib.gemm_bf16f32_nt(a, wt, z)
    assert torch.equal(mc.multi_margins(shard, w, k), z.reshape(-1))
    g = hiplib.gemm_bf16f32_tn(a, m.reshape(N, kc))
    assert torch.equal(mc.multi_grad(shard, m, k), _unpad(g, k))


def test_bf16_scoring_takes_the_split_gemms(monkeypatch):
    _clear_env(monkeypatch)
    k = 3
    shard, (w, _) = _dense(torch.bfloat16), _w_m(k)
    kc = mc.padded_k(k)
    wt = torch.zeros((kc, D), dtype=torch.float32, device=DEV)
    wt[:k] = w.reshape(D, k).T
    hi = wt.to(torch.bfloat16)
    lo = (wt - hi.to(torch.float32)).to(torch.bfloat16)
    z = torch.empty((N, kc), dtype=torch.float32, device=DEV)
    hiplib.gemm_bf16f32_nt(shard.features, hi, z)
    hiplib.gemm_bf16f32_nt(shard.features, lo, z, beta=1.0)
    assert torch.equal(mc.multi_margins(shard, w, k, scoring=True),
                       z.reshape(-1))


def test_f32_above_32_columns_takes_mm(monkeypatch):
    _clear_env(monkeypatch)
    k = 33
    shard, (w, m) = _dense(torch.float32), _w_m(k)
    a, kc = shard.features, mc.padded_k(k)
    z = torch.zeros((N, kc), device=DEV)
    z[:, :k] = a @ w.reshape(D, k)
    assert torch.equal(mc.multi_margins(shard, w, k), z.reshape(-1))
    g = (a.T @ m.reshape(N, kc)[:, :k]).reshape(-1)
    assert torch.equal(mc.multi_grad(shard, m, k), g)


@pytest.mark.parametrize("k,algo", [(33, None), (3, "mfma")])
def test_fp8_takes_the_mfma_kernels(k, algo, monkeypatch):
    _clear_env(monkeypatch)
    if algo:
        _set_env(monkeypatch, algo)
    shard, (w, m) = _dense(F8), _w_m(k)
    a = shard.features
    assert torch.equal(mc.multi_margins(shard, w, k),
                       ops.margins_multi_fp8(a, w, k))
    assert torch.equal(mc.multi_grad(shard, m, k),
                       ops.grad_multi_fp8(a, m, k, split_m=True))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, F8])
def test_valu_takes_the_valu_kernels(dtype, monkeypatch):
    _set_env(monkeypatch, "valu")
    k = 3
    shard, (w, m) = _dense(dtype), _w_m(k)
    a, kc = shard.features, mc.padded_k(k)
    assert torch.equal(mc.multi_margins(shard, w, k),
                       hiplib.dense_margins_multi(a, w, k, kc))
    assert torch.equal(mc.multi_grad(shard, m, k),
                       _unpad(hiplib.dense_grad_multi(a, m, kc), k))


@pytest.mark.parametrize("k", [3, 33])
def test_packed_takes_the_packed_kernels(k, monkeypatch):
    _clear_env(monkeypatch)
    monkeypatch.setattr(packing, "PACK_ESCAPE_CAP", 1.0)
    shard, (w, m) = _dense(torch.bfloat16, pack=True), _w_m(k)
    pk = shard._packed_gpu()
    assert pk is not None
    assert torch.equal(mc.multi_margins(shard, w, k),
                       ops.margins_multi_packed(pk, w, k))
    assert torch.equal(mc.multi_grad(shard, m, k),
                       ops.grad_multi_packed(pk, m, k, split_m=True))


@pytest.mark.parametrize("k", [3, 40])
def test_csr_takes_the_gather_kernels_per_chunk(k):
    shard, (w, m) = _csr(), _w_m(k)
    kc = mc.padded_k(k)
    colptr, crow, cval = shard.csc
    heavy = getattr(shard, "csc_heavy", None)
    w2, m2 = w.reshape(D, k), m.reshape(N, kc)
    z = torch.zeros((N, kc), device=DEV)
    g = torch.empty((D, k), device=DEV)
    for lo in range(0, k, 32):
        c = min(lo + 32, k) - lo
        kcc = mc.padded_k(c)
        zc = hiplib.csr_margins_multi(
            shard.rowptr, shard.col, shard.val,
            w2[:, lo:lo + c].reshape(-1), c, kcc, D)
        z[:, lo:lo + c] = zc.reshape(N, kcc)[:, :c]
        chunk = torch.zeros((N, kcc), device=DEV)
        chunk[:, :c] = m2[:, lo:lo + c]
        gc = hiplib.csc_grad_multi(colptr, crow, cval, chunk.reshape(-1), D,
                                   kcc, heavy)
        g[:, lo:lo + c] = gc.reshape(D, kcc)[:, :c]
    assert torch.equal(mc.multi_margins(shard, w, k), z.reshape(-1))
    assert torch.equal(mc.multi_grad(shard, m, k), g.reshape(-1))


# --- the two gradient classes share the route ---

def _shard_of(which, monkeypatch):
    if which == "csr":
        return _csr()
    if which == "packed":
        monkeypatch.setattr(packing, "PACK_ESCAPE_CAP", 1.0)
        return _dense(torch.bfloat16, pack=True)
    return _dense({"bf16": torch.bfloat16, "fp8": F8}[which])


@pytest.mark.parametrize("which,k,algo", [
    ("bf16", 3, None), ("bf16", 33, None), ("bf16", 3, "mfma"),
    ("bf16", 33, "mfma"), ("fp8", 33, None), ("packed", 3, None),
    ("packed", 33, None), ("csr", 3, None), ("csr", 40, None)])
def test_softmax_and_multitask_share_the_route(which, k, algo, monkeypatch):
    _clear_env(monkeypatch)
    if algo:
        _set_env(monkeypatch, algo)
    shard, (w, m) = _shard_of(which, monkeypatch), _w_m(k)
    softmax = MultinomialLogisticGradient(k)
    tasks = MultiTaskGradient(LogisticGradient(), k)
    z = softmax.margins(shard, w)
    assert torch.equal(z, tasks.margins(shard, w))
    # the same padded M into both: only the data pass differs by class
    lc = torch.zeros(2, dtype=torch.float64, device=DEV)
    for obj in (softmax, tasks):
        monkeypatch.setattr(obj, "multiplier_loss",
                            lambda shard, margins, mask=None: (m, lc))
    gs, _ = softmax.eval_from_margins(shard, z)
    gt, _ = tasks.eval_from_margins(shard, z)
    assert gs.numel() == D * k
    assert torch.equal(gs, gt)
    assert torch.equal(gs, mc.multi_grad(shard, m, k))
