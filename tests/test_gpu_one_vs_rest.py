"""One-vs-rest task multipliers (k_multiplier_tasks_ovr<KC>,
k_multiplier_tasks_ovr_anyk): every column bitwise against the binary kernel
on the relabelled vector, the whole call against the f64 oracle, and the
stacked evaluation against K binary evaluations."""

import functools

import pytest
import torch

from sparkagd_amd import CSRShard, DenseShard, LogisticGradient, MultiTaskGradient, ops
from sparkagd_amd.data import generate_csr_problem
from sparkagd_amd.ops import multitask as mt
from sparkagd_amd.ops.multiclass import padded_k

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOSSES = [ops.LOSS_LOGISTIC, ops.LOSS_LEAST_SQUARES, ops.LOSS_HINGE,
          ops.LOSS_SMOOTH_HINGE]
# (K, n): every KC template and its pads, the second grid-stride trip past
# the 1024-block cap (K = 32, n = 32800), the first width on the any-K kernel
# and its second 256-column chunk. "subset": the targets are a permuted strict
# subset of the classes. "extras": mask, {0.5, 1, 2} weights, folds, invert.
CASES = ([(k, n, "plain") for k, n in [(3, 1), (3, 67), (5, 67), (32, 67),
                                       (32, 32800), (33, 67), (260, 67)]]
         + [(5, 67, "subset"), (5, 67, "extras"), (33, 67, "extras")])


@functools.lru_cache(maxsize=None)
def _call(k, n, variant, loss_type):
    """Inputs (CPU) and the GPU one-vs-rest call of one case."""
    g = torch.Generator().manual_seed(1000 * n + 10 * k + loss_type)
    kc = padded_k(k)
    z = torch.full((n, kc), 7.0)  # junk in the pads must not leak
    z[:, :k] = 2.0 * torch.randn(n, k, generator=g)
    n_cls = 2 * k if variant == "subset" else k
    labels = torch.randint(0, n_cls, (n,), generator=g).to(torch.float32)
    target = torch.randperm(n_cls, generator=g)[:k].to(torch.int32)
    scale = (1.0 + torch.rand(k, generator=g)).to(torch.float32)
    extras, invert = (None,) * 4, False
    if variant == "extras":
        mask = (torch.rand(n, generator=g) < 0.7).to(torch.uint8)
        sw = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n,), generator=g)]
        fold = torch.randint(0, 3, (n,), generator=g, dtype=torch.int32)
        holdout = torch.tensor([(t % 4) - 1 for t in range(k)], dtype=torch.int32)
        extras, invert = (mask, sw, fold, holdout), True
    dev = [None if t is None else t.to(DEV) for t in extras]
    args = (z.reshape(-1).to(DEV), labels.to(DEV), loss_type, k, scale.to(DEV), *dev)
    out = mt.multiplier_tasks(*args, invert=invert, target=target.to(DEV))
    return (z, labels, target, scale, extras, invert), args, out


@pytest.mark.parametrize("loss_type", LOSSES)
@pytest.mark.parametrize("k,n,variant", CASES)
def test_columns_are_bitwise_the_binary_kernel(k, n, variant, loss_type):
    (z, labels, target, _, _, invert), args, (M, tl, lc) = _call(k, n, variant, loss_type)
    kc = padded_k(k)
    M2 = M.reshape(n, kc)
    assert torch.equal(M2[:, k:], torch.zeros_like(M2[:, k:]))
    for r in range(k):
        y = (labels == float(target[r])).to(torch.float32).to(DEV)
        Mb, tlb, lcb = mt.multiplier_tasks(args[0], y, *args[2:], invert=invert)
        assert torch.equal(M2[:, r], Mb.reshape(n, kc)[:, r]), r
        assert torch.equal(tl[r], tlb[r]), r
        assert torch.equal(lc[1], lcb[1])
    M_n, tl_n, lc_n = mt.multiplier_tasks(*args, invert=invert, need_mult=False,
                                          target=target.to(DEV))
    assert M_n is None
    assert torch.equal(tl, tl_n) and torch.equal(lc, lc_n)


@pytest.mark.parametrize("loss_type", LOSSES)
@pytest.mark.parametrize("k,n,variant", CASES)
def test_matches_f64_oracle(k, n, variant, loss_type):
    (z, labels, target, scale, extras, invert), _, (M, tl, lc) = _call(
        k, n, variant, loss_type)
    M_ref, tl_ref, lc_ref = mt.ref_multiplier_tasks(
        z[:, :k].double(), labels, loss_type, scale.double(), *extras,
        invert=invert, target=target)
    # the tolerances test_gpu_multitask.py holds k_multiplier_tasks to
    torch.testing.assert_close(M.reshape(n, -1)[:, :k].double().cpu(), M_ref,
                               rtol=3e-4, atol=3e-4)
    torch.testing.assert_close(tl.cpu(), tl_ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lc.cpu(), lc_ref, rtol=1e-5, atol=1e-5)


def _eval_shard(kind, labels):
    src, _ = generate_csr_problem(n=80, d=272, nnz_per_row=9, seed=3)
    if kind == "csr":
        return CSRShard(src.rowptr.to(DEV), src.col.to(DEV), src.val.to(DEV),
                        labels.to(DEV), src.d)
    dense = torch.sparse_csr_tensor(src.rowptr.long(), src.col.long(), src.val,
                                    size=(src.n, src.d)).to_dense()
    feats = dense + 0.1 * torch.randn(80, 272, generator=torch.Generator().manual_seed(4))
    return DenseShard(feats.to(DEV), labels.to(DEV))


@pytest.mark.parametrize("k", [3, 33])
@pytest.mark.parametrize("kind", ["dense", "csr"])
def test_eval_is_k_relabelled_binary_evals(kind, k):
    g = torch.Generator().manual_seed(k)
    labels = torch.randint(0, k, (80,), generator=g).to(torch.float32)
    w = (0.3 * torch.randn(272 * k, generator=g)).to(DEV)
    shard = _eval_shard(kind, labels)
    ovr = MultiTaskGradient(LogisticGradient(), k, target_class=range(k))
    grad, lc = ovr.eval(shard, w)
    loss = 0.0
    for c in range(k):
        sub = _eval_shard(kind, (labels == c).to(torch.float32))
        g_c, lc_c = LogisticGradient().eval(sub, w.reshape(-1, k)[:, c].contiguous())
        # f32 sums over n = 80 rows of O(1) terms in two summation orders,
        # from margins of two kernels: the multiplier test's 3e-4 covers it
        torch.testing.assert_close(grad.reshape(-1, k)[:, c], g_c.to(grad.dtype),
                                   rtol=3e-4, atol=3e-4)
        loss += float(lc_c[0])
    assert abs(float(lc[0]) - loss) <= 1e-5 * abs(loss)
    assert float(lc[1]) == 80.0
