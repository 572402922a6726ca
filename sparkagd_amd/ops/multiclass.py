"""Multinomial (softmax) logistic regression ops — oracle + dispatch.

A model family beyond the reference (MLlib 1.3's LogisticGradient is binary):
weights W [d, K] (stored flattened feature-major, classes contiguous),
margins Z [n, K] = A @ W, labels are class indices in {0..K-1}:

  p_i = softmax(z_i);  loss_i = logsumexp(z_i) - z_{i, y_i}
  M[i, k] = p_{i,k} - 1[y_i == k];  grad = Aᵀ M   (shape [d, K])

The GPU kernels work on a class dimension padded to KC = ceil(K/4)*4 (16-B
alignment of the per-feature class row); padding classes carry -inf margins
conceptually — implemented by restricting every softmax/loss loop to the
logical K, with padded multiplier columns exactly zero. Padding/unpadding
happens in this layer; callers only see the logical [d*K] / [n*K] flats.

Composes with the existing machinery: mini-batch masks, per-example sample
weights, and margin-state tracking (margins are linear in W and the prox
operators act elementwise on the flattened weights).
"""

from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

from . import (_use_hip, grad_multi_fp8, grad_multi_packed, hiplib,
               margins_multi_fp8, margins_multi_packed, multi_fp8_serves,
               multi_packed_serves, reference as _ref)


def _pad_classes(t2d: torch.Tensor, kc: int) -> torch.Tensor:
    n, k = t2d.shape
    if k == kc:
        return t2d.contiguous()
    out = torch.zeros((n, kc), dtype=t2d.dtype, device=t2d.device)
    out[:, :k] = t2d
    return out


def unpad_columns(gradp: torch.Tensor, k: int) -> torch.Tensor:
    """Logical flat [d*k] of a padded flat [d*KC] gradient."""
    kc = padded_k(k)
    if kc == k:
        return gradp
    return gradp.reshape(-1, kc)[:, :k].reshape(-1).contiguous()


def padded_k(k: int) -> int:
    """Class-dim padding: snapped to the VALU kernel template sizes
    (4/8/16/32) for small K; plain ceil-4 padding above 32, where the GPU
    path runs GEMM-shaped (hipBLASLt margins/grad + torch multiplier stage —
    bf16 or f32 shards) or, on fp8 shards, the fp8 MFMA kernels."""
    for kc in (4, 8, 16, 32):
        if k <= kc:
            return kc
    return (k + 3) // 4 * 4


# --- oracle (plain torch; CPU tier + GPU-kernel ground truth) ---

def ref_margins_multi(features: torch.Tensor, wflat: torch.Tensor, k: int) -> torch.Tensor:
    acc = torch.float32 if features.dtype in (torch.bfloat16, torch.float16, torch.float8_e4m3fn) else features.dtype
    w = wflat.reshape(features.shape[1], k).to(acc)
    return (features.to(acc) @ w).reshape(-1)  # flat [n*k]


def ref_eval_multi_from_margins(
    margins_flat: torch.Tensor,
    labels: torch.Tensor,
    features: torch.Tensor,
    k: int,
    mask: Optional[torch.Tensor] = None,
    need_grad: bool = True,
    sample_weight: Optional[torch.Tensor] = None,
) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    n = features.shape[0]
    z = margins_flat.reshape(n, k)
    acc = z.dtype
    y = labels.to(torch.int64)
    lse = torch.logsumexp(z, dim=1)
    zy = z.gather(1, y.unsqueeze(1)).squeeze(1)
    loss = lse - zy
    m = torch.softmax(z, dim=1)
    m = m.scatter_add(1, y.unsqueeze(1), -torch.ones((n, 1), dtype=acc, device=z.device))
    scale = torch.ones(n, dtype=acc, device=z.device)
    count_t = None
    if mask is not None:
        scale = scale * mask.to(acc)
    if sample_weight is not None:
        scale = scale * sample_weight.to(acc)
    if mask is not None or sample_weight is not None:
        loss = loss * scale
        m = m * scale.unsqueeze(1)
        count_t = scale.to(torch.float64).sum()
    if count_t is None:
        count_t = torch.tensor(float(n), dtype=torch.float64, device=z.device)
    loss_count = torch.stack([loss.to(torch.float64).sum(), count_t])
    if not need_grad:
        return None, loss_count
    facc = torch.float32 if features.dtype in (torch.bfloat16, torch.float16, torch.float8_e4m3fn) else features.dtype
    grad = (features.to(facc).T @ m.to(facc)).reshape(-1)  # flat [d*k]
    return grad, loss_count


def ref_eval_multi(features, labels, wflat, k, mask=None, need_grad=True,
                   sample_weight=None):
    zf = ref_margins_multi(features, wflat, k)
    return ref_eval_multi_from_margins(zf, labels, features, k, mask,
                                       need_grad, sample_weight)


def ref_multiplier_multi(
    z: torch.Tensor,  # [n, k] logical margins
    labels: torch.Tensor,
    mask: Optional[torch.Tensor] = None,
    sample_weight: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(M [n,k], loss_count f64[2]) — the n-space softmax multiplier stage."""
    n, k = z.shape
    acc = z.dtype
    y = labels.to(torch.int64)
    lse = torch.logsumexp(z, dim=1)
    loss = lse - z.gather(1, y.unsqueeze(1)).squeeze(1)
    m = torch.softmax(z, dim=1)
    m = m.scatter_add(1, y.unsqueeze(1),
                      -torch.ones((n, 1), dtype=acc, device=z.device))
    count_t = None
    if mask is not None or sample_weight is not None:
        scale = torch.ones(n, dtype=acc, device=z.device)
        if mask is not None:
            scale = scale * mask.to(acc)
        if sample_weight is not None:
            scale = scale * sample_weight.to(acc)
        loss = loss * scale
        m = m * scale.unsqueeze(1)
        count_t = scale.to(torch.float64).sum()
    if count_t is None:
        count_t = torch.tensor(float(n), dtype=torch.float64, device=z.device)
    return m, torch.stack([loss.to(torch.float64).sum(), count_t])


# --- CSR shards (oracle; GPU kernels are k_csr_margins_multi/k_csc_grad_multi) ---

def _csr_rows(rowptr: torch.Tensor) -> torch.Tensor:
    n = rowptr.numel() - 1
    counts = torch.diff(rowptr.to(torch.int64))
    return torch.repeat_interleave(
        torch.arange(n, device=rowptr.device, dtype=torch.int64), counts)


def ref_csr_margins_multi(rowptr, col, val, wflat, k: int, d: int) -> torch.Tensor:
    acc = torch.float32 if val.dtype in (torch.bfloat16, torch.float16) else val.dtype
    w = wflat.reshape(d, k).to(acc)
    n = rowptr.numel() - 1
    z = torch.zeros((n, k), dtype=acc, device=val.device)
    z.index_add_(0, _csr_rows(rowptr),
                 val.to(acc).unsqueeze(1) * w[col.to(torch.int64)])
    return z.reshape(-1)


def ref_csr_grad_multi(rowptr, col, val, m2d: torch.Tensor, d: int) -> torch.Tensor:
    acc = m2d.dtype
    grad = torch.zeros((d, m2d.shape[1]), dtype=acc, device=val.device)
    grad.index_add_(0, col.to(torch.int64),
                    val.to(acc).unsqueeze(1) * m2d[_csr_rows(rowptr)])
    return grad.reshape(-1)


# --- dispatch (GPU -> HIP kernels via hiplib; CPU -> oracle) ---

MULTI_ALGOS = ("auto", "gemm", "valu", "mfma")


def dense_multi_route(dtype: torch.dtype, kc: int, fp8_served: bool,
                      algo: str) -> str:
    """Backend of a multi-column data pass over a raw dense GPU block, for
    the margins Z = A·W and the gradient G = Aᵀ·M alike (the table of
    docs/KERNELS.md, first match wins):

      "gemm"      bf16 unless ``algo == "valu"``: hipBLASLt, the f32 operand
                  (W or M) rounded to bf16
      "mm"        f32 above 32 padded columns: rocBLAS through torch
      "fp8_mfma"  ``fp8_served`` (``multi_fp8_serves``) above 32 padded
                  columns, or at any width under ``algo == "mfma"``
      "valu"      the KC-templated exact-f32 kernels, ``kc <= 32``

    ``algo`` is the value of SPARKAGD_MULTI_MARGINS / SPARKAGD_MULTI_GRAD.
    "mfma" is defined for fp8 shards only; on any other block it means
    "auto". Pure: no tensor and no library is touched."""
    if algo not in MULTI_ALGOS:
        raise ValueError(
            f"SPARKAGD_MULTI_MARGINS / SPARKAGD_MULTI_GRAD must be one of "
            f"{', '.join(MULTI_ALGOS)}; got {algo!r}")
    if dtype == torch.bfloat16 and algo != "valu":
        return "gemm"
    if dtype == torch.float32 and kc > 32:
        return "mm"
    if fp8_served and (kc > 32 or algo == "mfma"):
        return "fp8_mfma"
    if kc <= 32:
        # VALU kernels are KC-templated <= 32
        return "valu"
    raise NotImplementedError(
        f"no multi-column kernel for KC={kc} > 32 on this {dtype} block under "
        f"algo={algo}: use a bf16 shard (hipBLASLt GEMM), an f32 shard "
        "(rocBLAS) or an fp8 shard with d % 16 == 0 (MFMA kernels)")


def _dense_route(features: torch.Tensor, k: int, grad: bool) -> str:
    """``dense_multi_route`` of a feature block; the one place that reads
    the two environment variables."""
    algo = (os.environ.get("SPARKAGD_MULTI_GRAD", "auto") if grad
            else os.environ.get("SPARKAGD_MULTI_MARGINS", "auto"))
    return dense_multi_route(features.dtype, padded_k(k),
                             multi_fp8_serves(features, k), algo)


def _gemm_margins_multi(features: torch.Tensor, wflat: torch.Tensor, k: int,
                        kc: int) -> torch.Tensor:
    """Margins as a skinny hipBLASLt GEMM: Z[n,KC] = A[n,d]·bf16(W)[d,KC].

    This is the idiomatic route for GEMM-shaped work — the per-element K-fma
    VALU kernel is load-issue bound at ~12x the A-stream floor for K=16
    (profiles/r01_multiclass_trace.txt). W is rounded to bf16 (the standard
    bf16 mixed-precision compute path; A is already bf16, accumulation f32);
    SPARKAGD_MULTI_MARGINS=valu selects the exact-f32-weights kernel instead.
    """
    n, d = features.shape
    wt = torch.zeros((kc, d), dtype=torch.bfloat16, device=features.device)
    wt[:k] = wflat.reshape(d, k).T.to(torch.bfloat16)
    z = torch.empty((n, kc), dtype=torch.float32, device=features.device)
    hiplib.gemm_bf16f32_nt(features, wt, z)
    return z.reshape(-1)


def _gemm_margins_scoring(features: torch.Tensor, wflat: torch.Tensor, k: int,
                          kc: int) -> torch.Tensor:
    """Margins of a bf16 block for SCORING returned weights. The training
    GEMM rounds W to bf16, a 2^-9 relative change of every weight: harmless
    inside the iteration, but a score must belong to the weights the caller
    gets back. Here W goes in as bf16(W) + bf16(W - bf16(W)), two
    accumulating hipBLASLt GEMMs (2^-17 per weight) at about twice the
    one-GEMM cost — the exact-f32 VALU kernel would cost ~12 A-streams.
    Every other route already multiplies the exact weights (the MFMA kernels
    carry W as bf16 hi + lo)."""
    n, d = features.shape
    wt = torch.zeros((kc, d), dtype=torch.float32, device=features.device)
    wt[:k] = wflat.reshape(d, k).T
    hi = wt.to(torch.bfloat16)
    lo = (wt - hi.to(torch.float32)).to(torch.bfloat16)
    z = torch.empty((n, kc), dtype=torch.float32, device=features.device)
    hiplib.gemm_bf16f32_nt(features, hi, z)
    hiplib.gemm_bf16f32_nt(features, lo, z, beta=1.0)
    return z.reshape(-1)


def margins_multi(features: torch.Tensor, wflat: torch.Tensor, k: int,
                  scoring: bool = False) -> torch.Tensor:
    """Flat padded margins [n*KC] of a dense block (opaque to callers; feed
    back into eval_multi_from_margins / axpby for margin tracking).
    ``scoring=True`` keeps the f32 weights of a bf16 GPU block
    (``_gemm_margins_scoring``)."""
    kc = padded_k(k)
    if not _use_hip(features):
        z = ref_margins_multi(features, wflat, k).reshape(features.shape[0], k)
        return _pad_classes(z, kc).reshape(-1)
    if scoring and features.dtype == torch.bfloat16:
        return _gemm_margins_scoring(features, wflat, k, kc)
    route = _dense_route(features, k, grad=False)
    if route == "gemm":
        return _gemm_margins_multi(features, wflat, k, kc)
    if route == "mm":
        # rocBLAS via torch.mm is the idiomatic f32 library GEMM
        z = features @ wflat.reshape(features.shape[1], k).to(torch.float32)
        return _pad_classes(z, kc).reshape(-1)
    if route == "fp8_mfma":
        return margins_multi_fp8(features, wflat, k)
    return hiplib.dense_margins_multi(features, wflat, k, kc)


def grad_from_mult_multi(features, m_padded_flat, k):
    """grad flat [d*k] = Aᵀ·M of a dense block from the padded multiplier."""
    kc = padded_k(k)
    n = features.shape[0]
    if not _use_hip(features):
        acc = (torch.float32 if features.dtype in
               (torch.bfloat16, torch.float16, torch.float8_e4m3fn)
               else features.dtype)
        m = m_padded_flat.reshape(n, kc)[:, :k].to(acc)
        return (features.to(acc).T @ m).reshape(-1)
    route = _dense_route(features, k, grad=True)
    if route == "gemm":
        # the per-element KC-fma VALU kernel is issue-bound ~3.5x the
        # A-stream floor (profiles/r01_multiclass_trace_gemm.txt). The
        # multipliers round to bf16 (standard mixed precision; A is bf16,
        # accumulation f32) and the pad columns of M are exact zeros;
        # SPARKAGD_MULTI_GRAD=valu selects the exact-f32-multiplier kernel.
        gradp = hiplib.gemm_bf16f32_tn(features, m_padded_flat.reshape(n, kc))
        return unpad_columns(gradp.reshape(-1), k)
    if route == "mm":
        return (features.T @ m_padded_flat.reshape(n, kc)[:, :k]).reshape(-1)
    if route == "fp8_mfma":
        # M as a bf16 hi + lo pair
        return grad_multi_fp8(features, m_padded_flat, k, split_m=True)
    return unpad_columns(hiplib.dense_grad_multi(features, m_padded_flat, kc), k)


def multiplier_loss_multi(labels, margins_padded_flat, k, mask=None,
                          sample_weight=None):
    """(M padded flat [n*KC] with exact-zero pad columns, loss_count f64[2])
    from padded margins — the n-space softmax stage, zero data passes (one
    kernel for every KC: templated <= 32, generic wave-per-row above)."""
    kc = padded_k(k)
    if _use_hip(margins_padded_flat):
        return hiplib.multiplier_multi(margins_padded_flat, labels, k, kc,
                                       mask, sample_weight)
    n = margins_padded_flat.numel() // kc
    z = margins_padded_flat.reshape(n, kc)[:, :k]
    m, lc = ref_multiplier_multi(z, labels, mask, sample_weight)
    return _pad_classes(m, kc).reshape(-1), lc


def eval_multi_from_margins(features, margins_padded_flat, labels, k,
                            mask=None, need_grad=True, sample_weight=None):
    M, loss_count = multiplier_loss_multi(labels, margins_padded_flat, k, mask,
                                          sample_weight)
    if not need_grad:
        return None, loss_count
    return grad_from_mult_multi(features, M, k), loss_count


def eval_multi(features, labels, wflat, k, mask=None, need_grad=True,
               sample_weight=None):
    zf = margins_multi(features, wflat, k)
    return eval_multi_from_margins(features, zf, labels, k, mask, need_grad,
                                   sample_weight)


# --- CSR shards ---

def csr_margins_multi(shard, wflat: torch.Tensor, k: int) -> torch.Tensor:
    """Flat padded margins [n*KC] over a CSRShard. K > 32 runs the KC=32
    gather kernel per 32-class chunk (the nnz stream re-reads per chunk —
    the K-proportional W/M traffic dominates anyway)."""
    kc = padded_k(k)
    if not _use_hip(shard.val):
        z = ref_csr_margins_multi(shard.rowptr, shard.col, shard.val, wflat, k,
                                  shard.d).reshape(-1, k)
        return _pad_classes(z, kc).reshape(-1)
    if kc <= 32:
        return hiplib.csr_margins_multi(shard.rowptr, shard.col, shard.val,
                                        wflat, k, kc, shard.d)
    n, d = shard.n, shard.d
    w2 = wflat.reshape(d, k).to(torch.float32)
    z = torch.zeros((n, kc), dtype=torch.float32, device=shard.val.device)
    for lo in range(0, k, 32):
        hi = min(lo + 32, k)
        wc = w2[:, lo:hi]
        zc = hiplib.csr_margins_multi(shard.rowptr, shard.col, shard.val,
                                      wc.reshape(-1), hi - lo,
                                      padded_k(hi - lo), d)
        z[:, lo:hi] = zc.reshape(n, padded_k(hi - lo))[:, : hi - lo]
    return z.reshape(-1)


def csr_grad_multi(shard, m_padded_flat: torch.Tensor, k: int) -> torch.Tensor:
    """grad flat [d*k] = Aᵀ·M on a CSRShard from the padded multiplier: the
    deterministic CSC gather (k_csc_grad_multi; 32-column chunks above
    KC = 32), the index_add oracle on CPU."""
    kc = padded_k(k)
    n = shard.n
    if not _use_hip(shard.val):
        m = m_padded_flat.reshape(n, kc)[:, :k]
        return ref_csr_grad_multi(shard.rowptr, shard.col, shard.val, m, shard.d)
    if shard.csc is None:
        raise RuntimeError(
            "the CSR multi-column gradient needs the deterministic CSC copy "
            "(CSRShard(..., deterministic=True))")
    colptr, crow, cval = shard.csc
    heavy = getattr(shard, "csc_heavy", None)
    if kc <= 32:
        return unpad_columns(
            hiplib.csc_grad_multi(colptr, crow, cval, m_padded_flat, shard.d,
                                  kc, heavy), k)
    m2d = m_padded_flat.reshape(n, kc)[:, :k]
    grad = torch.empty((shard.d, k), dtype=torch.float32,
                       device=shard.val.device)
    for lo in range(0, k, 32):
        hi = min(lo + 32, k)
        kcc = padded_k(hi - lo)
        chunk = torch.zeros((n, kcc), dtype=torch.float32,
                            device=shard.val.device)
        chunk[:, : hi - lo] = m2d[:, lo:hi]
        gc = hiplib.csc_grad_multi(colptr, crow, cval, chunk.reshape(-1),
                                   shard.d, kcc, heavy)
        grad[:, lo:hi] = gc.reshape(shard.d, kcc)[:, : hi - lo]
    return grad.reshape(-1).contiguous()


# --- the two data passes of a shard (softmax and multi-task alike) ---

def packed_copy_for(shard, k: int):
    """The shard's packed copy when the packed multi-column kernels serve it
    (a dense shard that already is packed, on the GPU, padded_k(k) <= 128),
    else None: the caller keeps the raw route."""
    if getattr(shard, "kind", None) != "dense":
        return None
    pk = shard._packed_gpu()
    return pk if multi_packed_serves(pk, k) else None


def multi_margins(shard, v: torch.Tensor, k: int,
                  scoring: bool = False) -> torch.Tensor:
    """Flat padded margins [n*KC] = A·V of a shard's rows for the [d, k]
    block ``v``: the CSR gather, the packed copy's MFMA kernel when it
    serves, else the raw dense block by ``dense_multi_route``. ``scoring``
    as in ``margins_multi``; CSR and packed passes carry the exact f32
    weights anyway (packed: W as bf16 hi + lo, one pass serves training and
    scoring)."""
    if getattr(shard, "kind", None) == "csr":
        return csr_margins_multi(shard, v, k)
    pk = packed_copy_for(shard, k)
    if pk is not None:
        return margins_multi_packed(pk, v, k)
    return margins_multi(shard.features, v, k, scoring)


def multi_grad(shard, m_padded_flat: torch.Tensor, k: int) -> torch.Tensor:
    """grad flat [d*k] = Aᵀ·M of a shard's rows from the padded multiplier
    [n*KC]; the ladder of ``multi_margins``. The packed kernel takes M as a
    bf16 hi + lo pair (``ops.grad_multi_packed`` says why)."""
    if getattr(shard, "kind", None) == "csr":
        return csr_grad_multi(shard, m_padded_flat, k)
    pk = packed_copy_for(shard, k)
    if pk is not None:
        return grad_multi_packed(pk, m_padded_flat, k, split_m=True)
    return grad_from_mult_multi(shard.features, m_padded_flat, k)


def multiclass_metrics(margins_padded_flat, labels, k, sample_weight=None):
    """(conf i64 [k, k], sums f64 [2], bad_labels, min_weight) from padded
    margins — one fused pass on GPU (k_multiclass_metrics), the oracle
    ``reference.multiclass_metrics`` on CPU."""
    kc = padded_k(k)
    if _use_hip(margins_padded_flat):
        return hiplib.multiclass_metrics(margins_padded_flat, labels, k, kc,
                                         sample_weight)
    return _ref.multiclass_metrics(margins_padded_flat, labels, k, kc,
                                   sample_weight)

