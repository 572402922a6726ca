"""ctypes binding to the CDNA4 kernel library (csrc/libagd_hip.so).

The .so is a plain C-ABI HIP library built directly by hipcc for gfx950 —
no hipify, no torch C++ headers, no pybind — loaded with ctypes and called
with raw device pointers plus torch's current HIP stream. The build lives
in-tree (``sparkagd_amd/csrc/libagd_hip.so``) so it travels with the repo
snapshot; ``__graft_entry__.build()`` produces it.

Determinism notes:
* the dense A^T·m path writes private partial slabs per (row-block,
  column-slab) workgroup and reduces them in a fixed order => bitwise
  reproducible gradients across runs (and therefore across ranks given
  identical inputs).
* the CSR A^T·m path is deterministic when the shard carries its CSC copy
  (the default: a gather kernel, no atomics). Without it an fp32 atomic
  scatter is used, whose summation order is non-deterministic at the
  rounding level; tests cross-check the two (SURVEY.md §5 'Race detection').
"""

from __future__ import annotations

import ctypes
import os
from typing import Optional, Tuple

import torch

_DTYPE_CODE = {torch.bfloat16: 0, torch.float32: 1, torch.float64: 2, torch.float8_e4m3fn: 3}
_ACC_DTYPE = {torch.bfloat16: torch.float32, torch.float32: torch.float32, torch.float64: torch.float64, torch.float8_e4m3fn: torch.float32}

_lib: Optional[ctypes.CDLL] = None

SO_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "csrc", "libagd_hip.so")


def so_path() -> str:
    return os.path.abspath(SO_PATH)


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    path = so_path()
    if not os.path.exists(path):
        raise FileNotFoundError(f"HIP kernel library not found at {path}")
    lib = ctypes.CDLL(path)

    lib.agd_last_error.restype = ctypes.c_char_p
    lib.agd_version.restype = ctypes.c_int
    lib.agd_dense_rowblocks.restype = ctypes.c_longlong
    lib.agd_dense_rowblocks.argtypes = [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int]
    lib.agd_margin_slabs.restype = ctypes.c_int
    lib.agd_margin_slabs.argtypes = [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int]

    P, LL, I, D = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_double
    lib.agd_dense_eval.restype = I
    lib.agd_dense_eval.argtypes = [P, I, P, P, P, P, LL, LL, P, P, P, P, P, LL, I, I, I, I, I, I, P, P]
    U = ctypes.c_uint
    lib.agd_dense_pack_hist_blocks.restype = I
    lib.agd_dense_pack_hist_blocks.argtypes = [LL, LL]
    lib.agd_dense_pack_hist.restype = I
    lib.agd_dense_pack_hist.argtypes = [P, LL, LL, P, P]
    lib.agd_dense_pack_encode.restype = I
    lib.agd_dense_pack_encode.argtypes = [P, LL, LL, U, U, P, P, P, P]
    lib.agd_dense_pack_escapes.restype = I
    lib.agd_dense_pack_escapes.argtypes = [P, LL, LL, U, U, P, P, P, P, P]
    lib.agd_dense_pack_row_words.restype = LL
    lib.agd_dense_pack_row_words.argtypes = [LL]
    lib.agd_dense_eval_packed.restype = I
    lib.agd_dense_eval_packed.argtypes = [P, U, U, P, P, P, P, P, P, LL, P, P, P, P, LL, LL,
                                          P, P, P, P, P, LL, I, I, I, I, I, P, P]
    lib.agd_dense_pack_row_bytes.restype = LL
    lib.agd_dense_pack_row_bytes.argtypes = [LL]
    lib.agd_dense_pack_decode.restype = I
    lib.agd_dense_pack_decode.argtypes = [P, U, U, P, P, P, LL, LL, LL, P, P]
    lib.agd_csr_eval.restype = I
    lib.agd_csr_eval.argtypes = [P, P, P, P, P, P, P, LL, LL, LL, P, P, P, P, I, P, P, P, I, I, P, P]
    lib.agd_axpby.restype = I
    lib.agd_axpby.argtypes = [D, P, D, P, P, LL, I, P]
    lib.agd_prox.restype = I
    lib.agd_prox.argtypes = [I, P, P, D, D, D, P, P, LL, I, P, P]
    lib.agd_fused_scalars.restype = I
    lib.agd_fused_scalars.argtypes = [P, P, P, P, P, LL, I, P, P]
    lib.agd_dot_diff.restype = I
    lib.agd_dot_diff.argtypes = [P, P, P, P, P, LL, I, P, P]
    lib.agd_gemm_bf16f32_nt.restype = I
    lib.agd_gemm_bf16f32_nt.argtypes = [P, P, P, LL, LL, LL, ctypes.c_float, P]
    lib.agd_gemm_bf16f32_tn.restype = I
    lib.agd_gemm_bf16f32_tn.argtypes = [P, P, P, LL, LL, LL, P]
    lib.agd_multi_rowblocks.restype = LL
    lib.agd_multi_rowblocks.argtypes = [LL, LL, I]
    lib.agd_margins_multi.restype = I
    lib.agd_margins_multi.argtypes = [P, I, P, LL, LL, I, P, P]
    lib.agd_multiplier_multi.restype = I
    lib.agd_multiplier_multi.argtypes = [P, P, P, P, LL, I, I, P, P, P, P]
    lib.agd_grad_multi.restype = I
    lib.agd_grad_multi.argtypes = [P, I, P, LL, LL, I, P, LL, P, P]
    lib.agd_csr_margins_multi.restype = I
    lib.agd_csr_margins_multi.argtypes = [P, P, P, P, LL, I, I, P, P]
    lib.agd_csc_grad_multi.restype = I
    lib.agd_csc_grad_multi.argtypes = [P, P, P, P, LL, I, P,
                                       I, P, P, P, LL, LL, I, P, P, P]
    lib.agd_csc_grad_skew.restype = I
    lib.agd_csc_grad_skew.argtypes = [P, P, P, P, LL, I, P, P, P, LL, LL, I, P, P, P, P]
    lib.agd_gram_mult_affine.restype = I
    lib.agd_gram_mult_affine.argtypes = [P, P, D, D, P, P, I, LL, P, P, P, P]
    lib.agd_gram_state_update.restype = I
    lib.agd_gram_state_update.argtypes = [P, P, P, P, D, D, D, D, LL, P, P, P, P, P, P]
    lib.agd_at_margin_update.restype = I
    lib.agd_at_margin_update.argtypes = [P, P, P, D, D, D, LL, I, P, P, P]
    lib.agd_colstats_rowblocks.restype = LL
    lib.agd_colstats_rowblocks.argtypes = [LL, LL, I]
    lib.agd_dense_colstats.restype = I
    lib.agd_dense_colstats.argtypes = [P, I, LL, LL, LL, P, P, P, P, P,
                                       P, P, P, P, P, I, P]
    lib.agd_csc_colstats.restype = I
    lib.agd_csc_colstats.argtypes = [P, P, LL, I, P, P, P, LL, LL, I,
                                     P, P, P, P, P, P, P, P, P, P, P]
    lib.agd_dense_scale_cols.restype = I
    lib.agd_dense_scale_cols.argtypes = [P, I, P, LL, LL, P, P]
    lib.agd_csr_scale_vals.restype = I
    lib.agd_csr_scale_vals.argtypes = [P, P, P, LL, P, P]
    lib.agd_csc_scale_vals.restype = I
    lib.agd_csc_scale_vals.argtypes = [P, P, P, LL, LL, P, P]
    lib.agd_metrics_max_blocks.restype = I
    lib.agd_metrics_max_blocks.argtypes = []
    lib.agd_binary_metrics.restype = I
    lib.agd_binary_metrics.argtypes = [P, I, P, P, P, I, D, LL, P, P, P, P, P]
    lib.agd_multiclass_metrics.restype = I
    lib.agd_multiclass_metrics.argtypes = [P, P, P, LL, I, I, P, P, P, P, P]
    lib.agd_multiplier_sum.restype = I
    lib.agd_multiplier_sum.argtypes = [P, P, P, P, I, LL, I, P, P, P, P]
    lib.agd_add_bias.restype = I
    lib.agd_add_bias.argtypes = [P, D, P, LL, LL, I, P]
    lib.agd_at_margin_update_off.restype = I
    lib.agd_at_margin_update_off.argtypes = [P, P, P, D, D, D, D, P, LL, LL, I,
                                             P, P, P]
    lib.agd_prox_free.restype = I
    lib.agd_prox_free.argtypes = [I, P, P, D, D, D, P, P, LL, LL, I, P, P]
    lib.agd_csr_grad_from_mult.restype = I
    lib.agd_csr_grad_from_mult.argtypes = [P, P, P, P, LL, LL, P, P, P, P, I,
                                           P, P, P, LL, LL, I, P, P, P]
    # multi-task family (ops/multitask.py)
    lib.agd_tasks_ws_doubles.restype = LL
    lib.agd_tasks_ws_doubles.argtypes = [I]
    lib.agd_multiplier_tasks.restype = I
    lib.agd_multiplier_tasks.argtypes = [P, P, P, P, P, P, P, I, I, LL, I, I,
                                         P, P, P, P, P]
    lib.agd_prox_tasks.restype = I
    lib.agd_prox_tasks.argtypes = [I, P, P, D, P, P, I, P, P, LL, I, P, P]
    lib.agd_at_margin_update_tasks.restype = I
    lib.agd_at_margin_update_tasks.argtypes = [P, P, P, D, P, D, LL, I, I, I,
                                               P, P, P]

    _lib = lib
    return lib


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"agd HIP kernel error rc={rc}: {_lib.agd_last_error().decode()}")


def _stream(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> Optional[ctypes.c_void_p]:
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


_red_ws_cache = {}


def _red_ws(device) -> torch.Tensor:
    """Per-device fp64 partials buffer for the two-stage scalar reductions
    (max grid 8192 x up to 5 accumulators)."""
    t = _red_ws_cache.get(device)
    if t is None:
        t = torch.empty(8192 * 5, dtype=torch.float64, device=device)
        _red_ws_cache[device] = t
    return t


def _prep_mask(mask: Optional[torch.Tensor], device) -> Optional[torch.Tensor]:
    if mask is None:
        return None
    if mask.dtype != torch.uint8:
        mask = mask.to(torch.uint8)
    return mask.contiguous().to(device)


def _prep_weights(sw: Optional[torch.Tensor], device) -> Optional[torch.Tensor]:
    if sw is None:
        return None
    if sw.dtype != torch.float32:
        sw = sw.to(torch.float32)
    return sw.contiguous().to(device)


def dense_eval(
    features: torch.Tensor,
    labels: torch.Tensor,
    w: torch.Tensor,
    loss_type: int,
    mask: Optional[torch.Tensor] = None,
    need_grad: bool = True,
    sample_weight: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    lib = load()
    assert features.is_cuda and features.is_contiguous() and features.ndim == 2
    n, d = features.shape
    a_dtype = _DTYPE_CODE[features.dtype]
    acc = _ACC_DTYPE[features.dtype]
    if w.dtype != acc:
        raise TypeError(f"weights dtype {w.dtype} must be {acc} for {features.dtype} features")
    w = w.contiguous()
    labels = labels.contiguous()
    if labels.dtype != torch.float32:
        labels = labels.to(torch.float32)
    mask = _prep_mask(mask, features.device)

    dev = features.device
    loss_count = torch.zeros(2, dtype=torch.float64, device=dev)
    # margins algorithm: 0 auto, 1 VALU row-group, 2 MFMA (bf16, d%16==0)
    margins_algo = int(os.environ.get("SPARKAGD_MARGINS_ALGO", "0"))
    n_slabs = int(lib.agd_margin_slabs(n, d, a_dtype, margins_algo))
    margins = torch.empty(n_slabs * n, dtype=acc, device=dev)
    mult = torch.empty(n, dtype=acc, device=dev)
    if need_grad:
        grad = torch.empty(d, dtype=acc, device=dev)
        n_rb = int(lib.agd_dense_rowblocks(n, d, a_dtype))
        part = torch.empty(n_rb * d, dtype=acc, device=dev) if n_rb > 1 else grad
    else:
        grad = part = None
        n_rb = 1

    sw = _prep_weights(sample_weight, features.device)
    rc = lib.agd_dense_eval(
        _ptr(features), a_dtype, _ptr(labels), _ptr(mask), _ptr(sw), _ptr(w),
        n, d, _ptr(grad), _ptr(loss_count), _ptr(margins), _ptr(mult),
        _ptr(part), n_rb, loss_type, n_slabs, 1 if need_grad else 0,
        margins_algo, int(os.environ.get("SPARKAGD_NT_LOADS", "1")),  # nt A-stream: +6-9% measured
        0, _ptr(_red_ws(features.device)), _stream(features),
    )
    _check(rc)
    return grad, loss_count


def dense_margins(features: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """margins = A @ v for an arbitrary d-vector (margin-state tracking)."""
    lib = load()
    assert features.is_cuda and features.is_contiguous() and features.ndim == 2
    n, d = features.shape
    a_dtype = _DTYPE_CODE[features.dtype]
    acc = _ACC_DTYPE[features.dtype]
    if v.dtype != acc:
        raise TypeError(f"vector dtype {v.dtype} must be {acc}")
    margins_algo = int(os.environ.get("SPARKAGD_MARGINS_ALGO", "0"))
    n_slabs = int(lib.agd_margin_slabs(n, d, a_dtype, margins_algo))
    margins = torch.empty(n_slabs * n, dtype=acc, device=features.device)
    rc = lib.agd_dense_eval(
        _ptr(features), a_dtype, None, None, None, _ptr(v.contiguous()),
        n, d, None, None, _ptr(margins), None, None, 1, 0, n_slabs, 0,
        margins_algo, int(os.environ.get("SPARKAGD_NT_LOADS", "1")),
        1, _ptr(_red_ws(features.device)), _stream(features),
    )
    _check(rc)
    return margins.narrow(0, 0, n)


def dense_eval_from_margins(
    features: torch.Tensor,
    margins: torch.Tensor,
    labels: torch.Tensor,
    loss_type: int,
    mask: Optional[torch.Tensor] = None,
    need_grad: bool = True,
    sample_weight: Optional[torch.Tensor] = None,
) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    """multiplier/loss (+ A^T·m when need_grad) from precomputed margins."""
    lib = load()
    assert features.is_cuda and features.is_contiguous() and features.ndim == 2
    n, d = features.shape
    a_dtype = _DTYPE_CODE[features.dtype]
    acc = _ACC_DTYPE[features.dtype]
    assert margins.dtype == acc and margins.numel() == n
    labels = labels.contiguous()
    if labels.dtype != torch.float32:
        labels = labels.to(torch.float32)
    mask = _prep_mask(mask, features.device)
    dev = features.device
    loss_count = torch.zeros(2, dtype=torch.float64, device=dev)
    mult = torch.empty(n, dtype=acc, device=dev)
    if need_grad:
        grad = torch.empty(d, dtype=acc, device=dev)
        n_rb = int(lib.agd_dense_rowblocks(n, d, a_dtype))
        part = torch.empty(n_rb * d, dtype=acc, device=dev) if n_rb > 1 else grad
    else:
        grad = part = None
        n_rb = 1
    sw = _prep_weights(sample_weight, features.device)
    rc = lib.agd_dense_eval(
        _ptr(features), a_dtype, _ptr(labels), _ptr(mask), _ptr(sw), None,
        n, d, _ptr(grad), _ptr(loss_count), _ptr(margins.contiguous()), _ptr(mult),
        _ptr(part), n_rb, loss_type, 1, 1 if need_grad else 0,
        1, int(os.environ.get("SPARKAGD_NT_LOADS", "1")),
        2, _ptr(_red_ws(features.device)), _stream(features),
    )
    _check(rc)
    return grad, loss_count


def dense_multiplier_loss(
    features: torch.Tensor,
    margins: torch.Tensor,
    labels: torch.Tensor,
    loss_type: int,
    mask: Optional[torch.Tensor] = None,
    sample_weight: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mult, loss_count) from precomputed margins — the Gram solver's
    n-space evaluation (no data pass at all)."""
    lib = load()
    n, d = features.shape
    a_dtype = _DTYPE_CODE[features.dtype]
    acc = _ACC_DTYPE[features.dtype]
    assert margins.dtype == acc and margins.numel() == n
    labels = labels.contiguous()
    if labels.dtype != torch.float32:
        labels = labels.to(torch.float32)
    mask = _prep_mask(mask, features.device)
    dev = features.device
    loss_count = torch.zeros(2, dtype=torch.float64, device=dev)
    mult = torch.empty(n, dtype=acc, device=dev)
    sw = _prep_weights(sample_weight, features.device)
    rc = lib.agd_dense_eval(
        _ptr(features), a_dtype, _ptr(labels), _ptr(mask), _ptr(sw), None,
        n, d, None, _ptr(loss_count), _ptr(margins.contiguous()), _ptr(mult),
        None, 1, loss_type, 1, 0,
        1, int(os.environ.get("SPARKAGD_NT_LOADS", "1")),
        2, _ptr(_red_ws(dev)), _stream(features),
    )
    _check(rc)
    return mult, loss_count


def dense_grad_from_mult(features: torch.Tensor, mult: torch.Tensor) -> torch.Tensor:
    """A^T @ mult for an arbitrary multiplier vector (Gram solver's final
    weight materialization)."""
    lib = load()
    n, d = features.shape
    a_dtype = _DTYPE_CODE[features.dtype]
    acc = _ACC_DTYPE[features.dtype]
    assert mult.dtype == acc and mult.numel() == n
    dev = features.device
    grad = torch.empty(d, dtype=acc, device=dev)
    n_rb = int(lib.agd_dense_rowblocks(n, d, a_dtype))
    part = torch.empty(n_rb * d, dtype=acc, device=dev) if n_rb > 1 else grad
    rc = lib.agd_dense_eval(
        _ptr(features), a_dtype, None, None, None, None,
        n, d, _ptr(grad), None, None, _ptr(mult.contiguous()),
        _ptr(part), n_rb, 0, 1, 1,
        1, int(os.environ.get("SPARKAGD_NT_LOADS", "1")),
        3, _ptr(_red_ws(dev)), _stream(features),
    )
    _check(rc)
    return grad


# --- 12-bit packed bf16 shard (one-time passes + packed stream) -----------

def dense_pack_hist(features: torch.Tensor) -> torch.Tensor:
    """[128] int64 (host) counts of the high-byte magnitude (bf16 bits 14..8)."""
    lib = load()
    assert features.is_cuda and features.is_contiguous() and features.dtype == torch.bfloat16
    n, d = features.shape
    blocks = int(lib.agd_dense_pack_hist_blocks(n, d))
    part = torch.empty((blocks, 128), dtype=torch.int64, device=features.device)
    _check(lib.agd_dense_pack_hist(_ptr(features), n, d, _ptr(part), _stream(features)))
    return part.sum(dim=0).cpu()


def dense_pack_encode(features: torch.Tensor, lut_lo: int, lut_hi: int):
    """(packed [n, row bytes] uint8, esc_count [n] int32, escape words
    [n, row groups / 64] int64: one bit per group) for the given table."""
    lib = load()
    n, d = features.shape
    row_bytes = int(lib.agd_dense_pack_row_bytes(d))
    packed = torch.empty((n, row_bytes), dtype=torch.uint8, device=features.device)
    esc_count = torch.empty(n, dtype=torch.int32, device=features.device)
    flags = torch.empty((n, int(lib.agd_dense_pack_row_words(d))), dtype=torch.int64,
                        device=features.device)
    _check(lib.agd_dense_pack_encode(_ptr(features), n, d, lut_lo, lut_hi,
                                     _ptr(packed), _ptr(esc_count), _ptr(flags),
                                     _stream(features)))
    return packed, esc_count, flags


def dense_pack_escapes(features: torch.Tensor, lut_lo: int, lut_hi: int,
                       flags: torch.Tensor, rowptr: torch.Tensor, nnz: int):
    """Row-sorted escape coordinates (col int32, val f32) for rowptr [n+1],
    from the escape words the encode pass wrote under the same table."""
    lib = load()
    n, d = features.shape
    col = torch.empty(nnz, dtype=torch.int32, device=features.device)
    val = torch.empty(nnz, dtype=torch.float32, device=features.device)
    _check(lib.agd_dense_pack_escapes(_ptr(features), n, d, lut_lo, lut_hi, _ptr(flags),
                                      _ptr(rowptr), _ptr(col), _ptr(val),
                                      _stream(features)))
    return col, val


def dense_pack_decode(pk, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The bf16 [n, d] matrix a PackedDense copy was built from, bit for bit
    (escapes included); ``out`` decodes into an existing buffer."""
    lib = load()
    dev = pk.packed.device
    assert pk.packed.is_cuda and pk.packed.is_contiguous()
    assert tuple(pk.packed.shape) == (pk.n, int(lib.agd_dense_pack_row_bytes(pk.d)))
    if out is None:
        out = torch.empty((pk.n, pk.d), dtype=torch.bfloat16, device=dev)
    assert (out.dtype == torch.bfloat16 and out.device == dev
            and tuple(out.shape) == (pk.n, pk.d) and out.is_contiguous())
    e = pk.esc
    _check(lib.agd_dense_pack_decode(
        _ptr(pk.packed), pk.lut_lo, pk.lut_hi, _ptr(e["rowptr"]),
        _ptr(e["col"]), _ptr(e["val"]), pk.nnz, pk.n, pk.d, _ptr(out),
        _stream(pk.packed)))
    return out


def _packed_call(pk, mode: int, *, w=None, labels=None, mask=None, sw=None,
                 margins=None, mult=None, loss_type: int = 0,
                 need_grad: bool = True):
    """agd_dense_eval modes 0-3 on a PackedDense copy (same planning and
    workspaces as the raw bf16 shard)."""
    lib = load()
    n, d = pk.n, pk.d
    dev = pk.packed.device
    acc = torch.float32
    n_slabs = int(lib.agd_margin_slabs(n, d, 0, 1)) if mode in (0, 1) else 1
    if mode in (0, 1):
        margins = torch.empty(n_slabs * n, dtype=acc, device=dev)
    loss_count = None
    if mode != 1 and mode != 3:
        loss_count = torch.zeros(2, dtype=torch.float64, device=dev)
    if mode in (0, 2):
        mult = torch.empty(n, dtype=acc, device=dev)
    grad = part = None
    n_rb = 1
    if need_grad and mode != 1:
        grad = torch.empty(d, dtype=acc, device=dev)
        n_rb = int(lib.agd_dense_rowblocks(n, d, 0))
        part = torch.empty(n_rb * d, dtype=acc, device=dev) if n_rb > 1 else grad
    e = pk.esc
    rc = lib.agd_dense_eval_packed(
        _ptr(pk.packed), pk.lut_lo, pk.lut_hi,
        _ptr(e["rowptr"]), _ptr(e["col"]), _ptr(e["val"]),
        _ptr(e["colptr"]), _ptr(e["row"]), _ptr(e["cval"]), pk.nnz,
        _ptr(labels), _ptr(mask), _ptr(sw), _ptr(w), n, d, _ptr(grad),
        _ptr(loss_count), _ptr(margins), _ptr(mult), _ptr(part), n_rb,
        loss_type, n_slabs, 1 if (need_grad and mode != 1) else 0,
        int(os.environ.get("SPARKAGD_NT_LOADS", "1")),
        mode, _ptr(_red_ws(dev)), _stream(pk.packed),
    )
    _check(rc)
    return grad, loss_count, margins


def _labels_f32(labels: torch.Tensor) -> torch.Tensor:
    labels = labels.contiguous()
    return labels if labels.dtype == torch.float32 else labels.to(torch.float32)


def dense_eval_packed(pk, labels, w, loss_type, mask=None, need_grad=True,
                      sample_weight=None):
    if w.dtype != torch.float32:
        raise TypeError(f"weights dtype {w.dtype} must be torch.float32 for a packed bf16 shard")
    dev = pk.packed.device
    grad, lc, _ = _packed_call(
        pk, 0, w=w.contiguous(), labels=_labels_f32(labels),
        mask=_prep_mask(mask, dev), sw=_prep_weights(sample_weight, dev),
        loss_type=loss_type, need_grad=need_grad)
    return grad, lc


def dense_margins_packed(pk, v: torch.Tensor) -> torch.Tensor:
    if v.dtype != torch.float32:
        raise TypeError(f"vector dtype {v.dtype} must be torch.float32")
    _, _, margins = _packed_call(pk, 1, w=v.contiguous(), need_grad=False)
    return margins.narrow(0, 0, pk.n)


def dense_eval_from_margins_packed(pk, margins, labels, loss_type, mask=None,
                                   need_grad=True, sample_weight=None):
    assert margins.dtype == torch.float32 and margins.numel() == pk.n
    dev = pk.packed.device
    grad, lc, _ = _packed_call(
        pk, 2, labels=_labels_f32(labels), mask=_prep_mask(mask, dev),
        sw=_prep_weights(sample_weight, dev), margins=margins.contiguous(),
        loss_type=loss_type, need_grad=need_grad)
    return grad, lc


def dense_grad_from_mult_packed(pk, mult: torch.Tensor) -> torch.Tensor:
    assert mult.dtype == torch.float32 and mult.numel() == pk.n
    grad, _, _ = _packed_call(pk, 3, mult=mult.contiguous(), need_grad=True)
    return grad


def _csc_grad_skew(csc, csc_heavy, mult: torch.Tensor, d: int) -> torch.Tensor:
    """Deterministic skew-robust CSC gradient: light thread-per-column pass
    for columns <= heavy_T nnz + wave-per-task partials for split heavy
    columns, combined in task order (agd_csc_grad_skew)."""
    lib = load()
    colptr, crow, cval = csc
    grad = torch.empty(d, dtype=torch.float32, device=cval.device)
    rc = lib.agd_csc_grad_skew(
        _ptr(colptr), _ptr(crow), _ptr(cval), _ptr(mult.contiguous()), d,
        int(csc_heavy["heavy_T"]), _ptr(csc_heavy["cols"]),
        _ptr(csc_heavy["taskptr"]), _ptr(csc_heavy["task_idx"]),
        csc_heavy["cols"].numel(), csc_heavy["task_idx"].numel(),
        int(csc_heavy["S"]), _ptr(csc_heavy["partial"]),
        _ptr(csc_heavy.get("order")), _ptr(grad),
        _stream(cval))
    _check(rc)
    return grad


def csr_eval(
    rowptr: torch.Tensor,
    col: torch.Tensor,
    val: torch.Tensor,
    labels: torch.Tensor,
    w: torch.Tensor,
    loss_type: int,
    mask: Optional[torch.Tensor] = None,
    d: Optional[int] = None,
    csc: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None,
    need_grad: bool = True,
    sample_weight: Optional[torch.Tensor] = None,
    csc_heavy: Optional[dict] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    lib = load()
    assert val.is_cuda and val.dtype == torch.float32
    if w.dtype != torch.float32:
        raise TypeError("CSR path requires float32 weights")
    n = rowptr.numel() - 1
    d = d if d is not None else w.numel()
    rowptr = rowptr.contiguous()
    col = col.contiguous()
    if rowptr.dtype != torch.int32:
        rowptr = rowptr.to(torch.int32)
    if col.dtype != torch.int32:
        col = col.to(torch.int32)
    labels = labels.contiguous()
    if labels.dtype != torch.float32:
        labels = labels.to(torch.float32)
    mask = _prep_mask(mask, val.device)

    dev = val.device
    if not need_grad:
        grad = None
        cp = cr = cv = None
    elif csc is None:
        grad = torch.zeros(d, dtype=torch.float32, device=dev)  # atomic path accumulates
        cp = cr = cv = None
    else:
        grad = torch.empty(d, dtype=torch.float32, device=dev)  # CSC path overwrites
        cp, cr, cv = csc
    loss_count = torch.zeros(2, dtype=torch.float64, device=dev)
    margins = torch.empty(n, dtype=torch.float32, device=dev)
    mult = torch.empty(n, dtype=torch.float32, device=dev)

    sw = _prep_weights(sample_weight, val.device)
    # skewed columns: let the C call stop after the multiplier, then run the
    # skew-robust gradient on the mult buffer
    skew = need_grad and csc is not None and csc_heavy is not None
    rc = lib.agd_csr_eval(
        _ptr(rowptr), _ptr(col), _ptr(val), _ptr(labels), _ptr(mask), _ptr(sw),
        _ptr(w.contiguous()), n, val.numel(), d, _ptr(grad), _ptr(loss_count),
        _ptr(margins), _ptr(mult), loss_type,
        _ptr(cp), _ptr(cr), _ptr(cv), 1 if (need_grad and not skew) else 0, 0,
        _ptr(_red_ws(val.device)), _stream(val),
    )
    _check(rc)
    if skew:
        grad = _csc_grad_skew(csc, csc_heavy, mult, d)
    return grad, loss_count


def dense_margins_multi(features: torch.Tensor, wflat: torch.Tensor, k: int,
                        kc: int) -> torch.Tensor:
    """Padded flat margins [n*KC] = A @ pad(W [d,K] -> [d,KC])."""
    lib = load()
    n, d = features.shape
    a_dtype = _DTYPE_CODE[features.dtype]
    if features.dtype == torch.float64:
        raise NotImplementedError("multi-class GPU path supports bf16/f32/f8 shards")
    dev = features.device
    w2 = wflat.reshape(d, k).to(torch.float32)
    if kc != k:
        wp = torch.zeros((d, kc), dtype=torch.float32, device=dev)
        wp[:, :k] = w2
    else:
        wp = w2.contiguous()
    Z = torch.empty(n * kc, dtype=torch.float32, device=dev)
    rc = lib.agd_margins_multi(_ptr(features), a_dtype, _ptr(wp), n, d, kc,
                               _ptr(Z), _stream(features))
    _check(rc)
    return Z


def multiplier_multi(
    margins_padded_flat: torch.Tensor,
    labels: torch.Tensor,
    k: int,
    kc: int,
    mask: Optional[torch.Tensor] = None,
    sample_weight: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(M [n*kc] f32, loss_count f64[2]) from padded softmax margins —
    the n-space multiplier stage shared by the dense and CSR paths."""
    lib = load()
    dev = margins_padded_flat.device
    n = margins_padded_flat.numel() // kc
    labels = labels.contiguous()
    if labels.dtype != torch.float32:
        labels = labels.to(torch.float32)
    mask = _prep_mask(mask, dev)
    sw = _prep_weights(sample_weight, dev)
    M = torch.empty(n * kc, dtype=torch.float32, device=dev)
    loss_count = torch.zeros(2, dtype=torch.float64, device=dev)
    rc = lib.agd_multiplier_multi(_ptr(margins_padded_flat.contiguous()),
                                  _ptr(labels), _ptr(mask), _ptr(sw), n, k, kc,
                                  _ptr(M), _ptr(loss_count),
                                  _ptr(_red_ws(dev)), _stream(margins_padded_flat))
    _check(rc)
    return M, loss_count


_tasks_ws_cache = {}


def _tasks_ws(device, kc: int) -> torch.Tensor:
    """Per-(device, KC) f64 partials of the task multiplier: KC + 1 per
    block, too many for ``_red_ws``; the library names the size."""
    t = _tasks_ws_cache.get((device, kc))
    if t is None:
        t = torch.empty(int(load().agd_tasks_ws_doubles(kc)),
                        dtype=torch.float64, device=device)
        _tasks_ws_cache[(device, kc)] = t
    return t


def multiplier_tasks(
    margins_padded_flat: torch.Tensor,
    labels: torch.Tensor,
    loss_type: int,
    r: int,
    kc: int,
    task_scale: torch.Tensor,
    mask: Optional[torch.Tensor] = None,
    sample_weight: Optional[torch.Tensor] = None,
    fold_id: Optional[torch.Tensor] = None,
    holdout: Optional[torch.Tensor] = None,
    invert: bool = False,
    need_mult: bool = True,
) -> Tuple[Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
    """(M [n*kc] f32 or None, task_loss f64[r], loss_count f64[2]) from padded
    margins of ``r`` binary tasks — the n-space stage of MultiTaskGradient."""
    lib = load()
    dev = margins_padded_flat.device
    if margins_padded_flat.dtype != torch.float32:
        raise NotImplementedError("multi-task GPU path carries f32 margins")
    n = margins_padded_flat.numel() // kc
    labels = labels.contiguous()
    if labels.dtype != torch.float32:
        labels = labels.to(torch.float32)
    mask = _prep_mask(mask, dev)
    sw = _prep_weights(sample_weight, dev)
    if fold_id is not None:
        fold_id = fold_id.to(device=dev, dtype=torch.int32).contiguous()
        if fold_id.numel() != n:
            raise ValueError("fold_id must be [n]")
    if holdout is not None:
        holdout = holdout.to(device=dev, dtype=torch.int32).contiguous()
        if holdout.numel() != r:
            raise ValueError("holdout must be [num_tasks]")
    task_scale = task_scale.to(device=dev, dtype=torch.float32).contiguous()
    if task_scale.numel() != r or labels.numel() != n:
        raise ValueError("task_scale must be [num_tasks] and labels [n]")
    M = (torch.empty(n * kc, dtype=torch.float32, device=dev)
         if need_mult else None)
    task_loss = torch.empty(r, dtype=torch.float64, device=dev)
    loss_count = torch.empty(2, dtype=torch.float64, device=dev)
    rc = lib.agd_multiplier_tasks(
        _ptr(margins_padded_flat.contiguous()), _ptr(labels), _ptr(mask),
        _ptr(sw), _ptr(fold_id), _ptr(holdout), _ptr(task_scale),
        int(loss_type), int(bool(invert)), n, r, kc, _ptr(M), _ptr(task_loss),
        _ptr(loss_count), _ptr(_tasks_ws(dev, kc)),
        _stream(margins_padded_flat))
    _check(rc)
    return M, task_loss, loss_count


def prox_tasks(kind: int, w: torch.Tensor, g: torch.Tensor, step: float,
               lam: torch.Tensor, lam2: torch.Tensor
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``prox`` over the flat feature-major [d, R] block with task r's
    (lam[r], lam2[r]); lam / lam2 are f64 [R] on w's device."""
    lib = load()
    r = lam.numel()
    if lam2.numel() != r or w.numel() % r != 0:
        raise ValueError("prox_tasks: weights must be [d * R] with lam, lam2 [R]")
    lam = lam.to(device=w.device, dtype=torch.float64).contiguous()
    lam2 = lam2.to(device=w.device, dtype=torch.float64).contiguous()
    out = torch.empty_like(w)
    reg = torch.zeros((), dtype=torch.float64, device=w.device)
    rc = lib.agd_prox_tasks(kind, _ptr(w.contiguous()), _ptr(g.contiguous()),
                            float(step), _ptr(lam), _ptr(lam2), r, _ptr(out),
                            _ptr(reg), w.numel(), _VEC_DTYPE[w.dtype],
                            _ptr(_red_ws(w.device)), _stream(w))
    _check(rc)
    return out, reg


def at_margin_update_tasks(zm_old: torch.Tensor, xm_old: torch.Tensor,
                           gm: torch.Tensor, step: float, lam: torch.Tensor,
                           theta: float, num_tasks: int, kc: int):
    """(zm_new, xm_new) of the padded [n*kc] margins with task r's shrink
    ``1 - step*lam[r]`` (k_at_margin_update_tasks); pad columns come out as
    exact zeros. lam is f64 [R]: already on the device it is used as it is
    (no copy, no synchronisation)."""
    lib = load()
    total = zm_old.numel()
    if total % kc != 0 or xm_old.numel() != total or gm.numel() != total:
        raise ValueError("at_margin_update_tasks: margins must be three "
                         f"[n * {kc}] flats")
    if xm_old.dtype != zm_old.dtype or gm.dtype != zm_old.dtype:
        raise TypeError("at_margin_update_tasks: margins must share one dtype")
    if lam.numel() != num_tasks:
        raise ValueError("at_margin_update_tasks: lam must be [num_tasks]")
    lam = lam.to(device=zm_old.device, dtype=torch.float64).contiguous()
    zm_new = torch.empty_like(zm_old)
    xm_new = torch.empty_like(xm_old)
    rc = lib.agd_at_margin_update_tasks(
        _ptr(zm_old.contiguous()), _ptr(xm_old.contiguous()),
        _ptr(gm.contiguous()), float(step), _ptr(lam), float(theta),
        total // kc, int(num_tasks), int(kc), _VEC_DTYPE[zm_old.dtype],
        _ptr(zm_new), _ptr(xm_new), _stream(zm_old))
    _check(rc)
    return zm_new, xm_new


def dense_eval_multi_from_margins(
    features: torch.Tensor,
    margins_padded_flat: torch.Tensor,
    labels: torch.Tensor,
    k: int,
    kc: int,
    mask: Optional[torch.Tensor] = None,
    need_grad: bool = True,
    sample_weight: Optional[torch.Tensor] = None,
) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    lib = load()
    n, d = features.shape
    a_dtype = _DTYPE_CODE[features.dtype]
    dev = features.device
    M, loss_count = multiplier_multi(margins_padded_flat, labels, k, kc, mask,
                                     sample_weight)
    if not need_grad:
        return None, loss_count
    algo = os.environ.get("SPARKAGD_MULTI_GRAD", "auto")
    if features.dtype == torch.bfloat16 and algo in ("auto", "gemm"):
        # grad = A^T·M as a skinny hipBLASLt TN GEMM — the per-element KC-fma
        # VALU kernel is issue-bound ~3.5x the A-stream floor
        # (profiles/r01_multiclass_trace_gemm.txt). Multipliers round to bf16
        # (standard mixed precision; A is bf16, accumulation f32);
        # SPARKAGD_MULTI_GRAD=valu selects the exact-f32-multiplier kernel.
        gradp = gemm_bf16f32_tn(features, M.reshape(n, kc)).reshape(-1)
    else:
        n_rb = int(lib.agd_multi_rowblocks(n, d, kc))
        gradp = torch.empty(d * kc, dtype=torch.float32, device=dev)
        part = torch.empty(n_rb * d * kc, dtype=torch.float32, device=dev) if n_rb > 1 else gradp
        rc = lib.agd_grad_multi(_ptr(features), a_dtype, _ptr(M), n, d, kc,
                                _ptr(part), n_rb, _ptr(gradp), _stream(features))
        _check(rc)
    if kc != k:
        grad = gradp.reshape(d, kc)[:, :k].reshape(-1).contiguous()
    else:
        grad = gradp
    return grad, loss_count


def csr_margins_multi(rowptr, col, val, wflat: torch.Tensor, k: int,
                      kc: int, d: int) -> torch.Tensor:
    """Padded flat margins [n*KC] = CSR(A) @ pad(W [d,K] -> [d,KC]).

    SPARKAGD_CSR_MULTI_W=bf16 gathers bf16-rounded W rows (half the gather
    bytes, double the effective LLC coverage of W — the pass is
    LLC-miss-bound once W exceeds the last-level cache); default f32 keeps
    exact weights (the CSR values are f32)."""
    lib = load()
    n = rowptr.numel() - 1
    dev = val.device
    wdt = (torch.bfloat16
           if os.environ.get("SPARKAGD_CSR_MULTI_W", "f32") == "bf16"
           else torch.float32)
    w2 = wflat.reshape(d, k).to(wdt)
    if kc != k:
        wp = torch.zeros((d, kc), dtype=wdt, device=dev)
        wp[:, :k] = w2
    else:
        wp = w2.contiguous()
    Z = torch.empty(n * kc, dtype=torch.float32, device=dev)
    rowptr, col = _csr_idx(rowptr, col)
    rc = lib.agd_csr_margins_multi(_ptr(rowptr), _ptr(col),
                                   _ptr(val.contiguous()), _ptr(wp), n, kc,
                                   0 if wdt == torch.bfloat16 else 1,
                                   _ptr(Z), _stream(val))
    _check(rc)
    return Z


def csc_grad_multi(colptr, row, cval, M: torch.Tensor, d: int,
                   kc: int, csc_heavy: Optional[dict] = None) -> torch.Tensor:
    """grad flat [d*KC] = A^T·M via the deterministic CSC gather; skewed
    columns (csc_heavy, built by CSRShard) run the wave-per-task split."""
    lib = load()
    grad = torch.empty(d * kc, dtype=torch.float32, device=cval.device)
    if csc_heavy is not None:
        n_tasks = csc_heavy["task_idx"].numel()
        partial = (torch.empty(n_tasks * kc, dtype=torch.float32,
                               device=cval.device) if n_tasks > 0 else None)
        rc = lib.agd_csc_grad_multi(
            _ptr(colptr.contiguous()), _ptr(row.contiguous()),
            _ptr(cval.contiguous()), _ptr(M.contiguous()), d, kc, _ptr(grad),
            int(csc_heavy["heavy_T"]), _ptr(csc_heavy["cols"]),
            _ptr(csc_heavy["taskptr"]), _ptr(csc_heavy["task_idx"]),
            csc_heavy["cols"].numel(), n_tasks, int(csc_heavy["S"]),
            _ptr(partial), _ptr(csc_heavy.get("order")), _stream(cval))
    else:
        rc = lib.agd_csc_grad_multi(
            _ptr(colptr.contiguous()), _ptr(row.contiguous()),
            _ptr(cval.contiguous()), _ptr(M.contiguous()), d, kc, _ptr(grad),
            0, None, None, None, 0, 0, 0, None, None, _stream(cval))
    _check(rc)
    return grad


def gemm_bf16f32_nt(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor,
                    beta: float = 0.0) -> torch.Tensor:
    """C[m,n] (f32) = A[m,k] (bf16) @ B[n,k]^T (bf16) + beta*C via hipBLASLt
    (fp32 accumulation, fp32 output — used by the Gram-operator build)."""
    lib = load()
    assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16
    assert C.dtype == torch.float32
    m, k = A.shape
    n, k2 = B.shape
    assert k == k2 and C.shape == (m, n)
    assert A.is_contiguous() and B.is_contiguous() and C.is_contiguous()
    rc = lib.agd_gemm_bf16f32_nt(_ptr(A), _ptr(B), _ptr(C), m, n, k,
                                 float(beta), _stream(A))
    _check(rc)
    return C


def gemm_bf16f32_tn(A: torch.Tensor, M: torch.Tensor) -> torch.Tensor:
    """grad[d,kc] (f32) = A[n,d]^T (bf16) @ M[n,kc] (bf16-rounded) via
    hipBLASLt — the multinomial gradient GEMM (fp32 accumulation). Accepts M
    in f32 (rounded here) or bf16; works for any kc."""
    lib = load()
    assert A.dtype == torch.bfloat16
    n, d = A.shape
    n2, kc = M.shape
    assert n == n2
    if M.dtype != torch.bfloat16:
        M = M.to(torch.bfloat16)
    M = M.contiguous()
    grad = torch.empty((d, kc), dtype=torch.float32, device=A.device)
    rc = lib.agd_gemm_bf16f32_tn(_ptr(A.contiguous()), _ptr(M), _ptr(grad),
                                 n, d, kc, _stream(A))
    _check(rc)
    return grad


def _csr_idx(rowptr: torch.Tensor, col: torch.Tensor):
    """Kernel index arrays are int32: convert int64 inputs (no-op otherwise).
    Passing int64 straight through would silently misread (the bug the
    MixedShard GPU test caught in round 2)."""
    rowptr = rowptr.contiguous()
    col = col.contiguous()
    if rowptr.dtype != torch.int32:
        rowptr = rowptr.to(torch.int32)
    if col.dtype != torch.int32:
        col = col.to(torch.int32)
    return rowptr, col


def csr_margins(rowptr, col, val, v: torch.Tensor) -> torch.Tensor:
    lib = load()
    n = rowptr.numel() - 1
    rowptr, col = _csr_idx(rowptr, col)
    margins = torch.empty(n, dtype=torch.float32, device=val.device)
    rc = lib.agd_csr_eval(
        _ptr(rowptr), _ptr(col), _ptr(val.contiguous()),
        None, None, None, _ptr(v.contiguous()), n, val.numel(), v.numel(),
        None, None, _ptr(margins), None, 0, None, None, None, 0, 1,
        _ptr(_red_ws(val.device)), _stream(val),
    )
    _check(rc)
    return margins


def csr_eval_from_margins(rowptr, col, val, margins, labels, loss_type,
                          mask=None, d=None, csc=None, need_grad=True,
                          sample_weight=None, csc_heavy=None):
    lib = load()
    n = rowptr.numel() - 1
    rowptr, col = _csr_idx(rowptr, col)
    d = d if d is not None else 0
    labels = labels.contiguous()
    if labels.dtype != torch.float32:
        labels = labels.to(torch.float32)
    mask = _prep_mask(mask, val.device)
    dev = val.device
    if not need_grad:
        grad = None; cp = cr = cv = None
    elif csc is None:
        grad = torch.zeros(d, dtype=torch.float32, device=dev); cp = cr = cv = None
    else:
        grad = torch.empty(d, dtype=torch.float32, device=dev); cp, cr, cv = csc
    loss_count = torch.zeros(2, dtype=torch.float64, device=dev)
    mult = torch.empty(n, dtype=torch.float32, device=dev)
    sw = _prep_weights(sample_weight, val.device)
    skew = need_grad and csc is not None and csc_heavy is not None
    rc = lib.agd_csr_eval(
        _ptr(rowptr), _ptr(col), _ptr(val.contiguous()),
        _ptr(labels), _ptr(mask), _ptr(sw), None, n, val.numel(), d,
        _ptr(grad), _ptr(loss_count), _ptr(margins.contiguous()), _ptr(mult),
        loss_type, _ptr(cp), _ptr(cr), _ptr(cv),
        1 if (need_grad and not skew) else 0, 2,
        _ptr(_red_ws(val.device)), _stream(val),
    )
    _check(rc)
    if skew:
        grad = _csc_grad_skew(csc, csc_heavy, mult, d)
    return grad, loss_count


_VEC_DTYPE = {torch.float32: 1, torch.float64: 2}


def axpby(a: float, x: torch.Tensor, b: float, y: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = load()
    if out is None:
        out = torch.empty_like(x)
    rc = lib.agd_axpby(float(a), _ptr(x.contiguous()), float(b), _ptr(y.contiguous()),
                       _ptr(out), x.numel(), _VEC_DTYPE[x.dtype], _stream(x))
    _check(rc)
    return out


def prox(kind: int, w: torch.Tensor, g: torch.Tensor, step: float, lam: float,
         lam2: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    lib = load()
    out = torch.empty_like(w)
    reg = torch.zeros((), dtype=torch.float64, device=w.device)
    rc = lib.agd_prox(kind, _ptr(w.contiguous()), _ptr(g.contiguous()), float(step),
                      float(lam), float(lam2), _ptr(out), _ptr(reg), w.numel(),
                      _VEC_DTYPE[w.dtype], _ptr(_red_ws(w.device)), _stream(w))
    _check(rc)
    return out, reg


def fused_scalars(x: torch.Tensor, y: torch.Tensor, g_y: torch.Tensor, x_old: torch.Tensor) -> torch.Tensor:
    lib = load()
    out = torch.zeros(5, dtype=torch.float64, device=x.device)
    rc = lib.agd_fused_scalars(_ptr(x.contiguous()), _ptr(y.contiguous()),
                               _ptr(g_y.contiguous()), _ptr(x_old.contiguous()),
                               _ptr(out), x.numel(), _VEC_DTYPE[x.dtype],
                               _ptr(_red_ws(x.device)), _stream(x))
    _check(rc)
    return out


def dot_diff(x: torch.Tensor, y: torch.Tensor, g_x: torch.Tensor, g_y: torch.Tensor) -> torch.Tensor:
    lib = load()
    out = torch.zeros((), dtype=torch.float64, device=x.device)
    rc = lib.agd_dot_diff(_ptr(x.contiguous()), _ptr(y.contiguous()),
                          _ptr(g_x.contiguous()), _ptr(g_y.contiguous()),
                          _ptr(out), x.numel(), _VEC_DTYPE[x.dtype],
                          _ptr(_red_ws(x.device)), _stream(x))
    _check(rc)
    return out


def gram_mult_affine(xm: torch.Tensor, zm: torch.Tensor, a: float, b: float,
                     labels: torch.Tensor, loss_type: int,
                     sample_weight: Optional[torch.Tensor] = None,
                     mult_out: Optional[torch.Tensor] = None,
                     lc_out: Optional[torch.Tensor] = None):
    """(mult, loss_count) at margins a*xm + b*zm without materializing the
    combination — the Gram solver's fused y-evaluation (binary losses,
    full batch)."""
    lib = load()
    n = xm.numel()
    dev = xm.device
    labels = labels.contiguous()
    if labels.dtype != torch.float32:
        labels = labels.to(torch.float32)
    mult = mult_out if mult_out is not None else torch.empty(
        n, dtype=torch.float32, device=dev)
    lc = lc_out if lc_out is not None else torch.empty(
        2, dtype=torch.float64, device=dev)
    lc.zero_()
    sw = _prep_weights(sample_weight, dev)
    rc = lib.agd_gram_mult_affine(_ptr(xm.contiguous()), _ptr(zm.contiguous()),
                                  float(a), float(b), _ptr(labels), _ptr(sw),
                                  loss_type, n, _ptr(mult), _ptr(lc),
                                  _ptr(_red_ws(dev)), _stream(xm))
    _check(rc)
    return mult, lc


def gram_state_update(gm_raw: torch.Tensor, m_y: torch.Tensor,
                      xm_old: torch.Tensor, zm_old: torch.Tensor,
                      inv_c: float, theta: float, pz: float, pg: float,
                      xb_t: torch.Tensor, md: torch.Tensor,
                      mstore_t: torch.Tensor, zm_new: torch.Tensor,
                      xm_new: torch.Tensor) -> None:
    """One fused pass finishing a Gram basis registration + the AT margin
    updates (see k_gram_state_update)."""
    lib = load()
    rc = lib.agd_gram_state_update(
        _ptr(gm_raw.contiguous()), _ptr(m_y.contiguous()),
        _ptr(xm_old.contiguous()), _ptr(zm_old.contiguous()),
        float(inv_c), float(theta), float(pz), float(pg), gm_raw.numel(),
        _ptr(xb_t), _ptr(md), _ptr(mstore_t), _ptr(zm_new), _ptr(xm_new),
        _stream(gm_raw))
    _check(rc)


def at_margin_update(zm_old: torch.Tensor, xm_old: torch.Tensor,
                     gm: torch.Tensor, pz: float, pg: float, theta: float):
    """(zm_new, xm_new) = (pz*zm + pg*gm, (1-theta)*xm + theta*zm_new) in one
    fused pass (direct tracked path)."""
    lib = load()
    zm_new = torch.empty_like(zm_old)
    xm_new = torch.empty_like(xm_old)
    rc = lib.agd_at_margin_update(
        _ptr(zm_old.contiguous()), _ptr(xm_old.contiguous()),
        _ptr(gm.contiguous()), float(pz), float(pg), float(theta),
        zm_old.numel(), _VEC_DTYPE[zm_old.dtype], _ptr(zm_new), _ptr(xm_new),
        _stream(zm_old))
    _check(rc)
    return zm_new, xm_new


# ---------------------------------------------------------------------------
# Native intercept (weights [w; b], bias last): n-space kernels only
# ---------------------------------------------------------------------------

def _bias_src(src: torch.Tensor, idx: int, like: torch.Tensor) -> torch.Tensor:
    """The device vector a bias is read from, checked against the vector it
    is applied to (same dtype and device, index in range)."""
    if src.dtype != like.dtype or src.device != like.device:
        raise TypeError(
            f"bias source ({src.dtype}, {src.device}) must match the margins "
            f"({like.dtype}, {like.device})")
    if not 0 <= idx < src.numel():
        raise IndexError(f"bias index {idx} outside [0, {src.numel()})")
    return src.contiguous()


def multiplier_loss_sum(
    margins: torch.Tensor,
    labels: torch.Tensor,
    loss_type: int,
    mask: Optional[torch.Tensor] = None,
    sample_weight: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mult [n], f64[3] = {loss, count, Σmult}) from margins
    (k_multiplier_sum): the multiplier stage plus the bias gradient."""
    lib = load()
    if margins.dtype not in _VEC_DTYPE:
        raise TypeError(f"margins must be f32 or f64, got {margins.dtype}")
    dev = margins.device
    n = margins.numel()
    labels = labels.contiguous()
    if labels.dtype != torch.float32:
        labels = labels.to(torch.float32)
    mask = _prep_mask(mask, dev)
    sw = _prep_weights(sample_weight, dev)
    mult = torch.empty(n, dtype=margins.dtype, device=dev)
    out = torch.zeros(3, dtype=torch.float64, device=dev)
    rc = lib.agd_multiplier_sum(
        _ptr(margins.contiguous()), _ptr(labels), _ptr(mask), _ptr(sw),
        loss_type, n, _VEC_DTYPE[margins.dtype], _ptr(mult), _ptr(out),
        _ptr(_red_ws(dev)), _stream(margins))
    _check(rc)
    return mult, out


def add_bias_(margins: torch.Tensor, coef: float, src: torch.Tensor,
              idx: int) -> torch.Tensor:
    """In place margins += coef * src[idx], the bias read on the device."""
    lib = load()
    if not margins.is_contiguous():
        raise ValueError("add_bias_ needs contiguous margins")
    src = _bias_src(src, idx, margins)
    rc = lib.agd_add_bias(_ptr(margins), float(coef), _ptr(src), idx,
                          margins.numel(), _VEC_DTYPE[margins.dtype],
                          _stream(margins))
    _check(rc)
    return margins


def at_margin_update_off(zm_old: torch.Tensor, xm_old: torch.Tensor,
                         gm: torch.Tensor, pz: float, pg: float, theta: float,
                         coef: float, src: torch.Tensor, idx: int):
    """at_margin_update with the constant term coef * src[idx] added to zm'
    (k_at_margin_update_off)."""
    lib = load()
    src = _bias_src(src, idx, zm_old)
    zm_new = torch.empty_like(zm_old)
    xm_new = torch.empty_like(xm_old)
    rc = lib.agd_at_margin_update_off(
        _ptr(zm_old.contiguous()), _ptr(xm_old.contiguous()),
        _ptr(gm.contiguous()), float(pz), float(pg), float(theta),
        float(coef), _ptr(src), idx, zm_old.numel(),
        _VEC_DTYPE[zm_old.dtype], _ptr(zm_new), _ptr(xm_new), _stream(zm_old))
    _check(rc)
    return zm_new, xm_new


def prox_free(kind: int, w: torch.Tensor, g: torch.Tensor, step: float,
              lam: float, lam2: float, n_free: int
              ) -> Tuple[torch.Tensor, torch.Tensor]:
    """prox whose last n_free coordinates take the plain gradient step and
    stay out of the regularisation value (k_prox_free)."""
    lib = load()
    if not 0 <= n_free <= w.numel():
        raise ValueError(f"n_free {n_free} outside [0, {w.numel()}]")
    out = torch.empty_like(w)
    reg = torch.zeros((), dtype=torch.float64, device=w.device)
    rc = lib.agd_prox_free(kind, _ptr(w.contiguous()), _ptr(g.contiguous()),
                           float(step), float(lam), float(lam2), _ptr(out),
                           _ptr(reg), w.numel(), int(n_free),
                           _VEC_DTYPE[w.dtype], _ptr(_red_ws(w.device)),
                           _stream(w))
    _check(rc)
    return out, reg


def csr_grad_from_mult(rowptr, col, val, mult: torch.Tensor, d: int,
                       csc=None, csc_heavy: Optional[dict] = None
                       ) -> torch.Tensor:
    """A^T @ mult for a CSR shard: the deterministic CSC gather when ``csc``
    is given (heavy columns through the shard's task split), the fp32 atomic
    scatter otherwise."""
    lib = load()
    assert val.is_cuda and val.dtype == torch.float32
    n = rowptr.numel() - 1
    if mult.dtype != torch.float32 or mult.numel() != n:
        raise TypeError("CSR multiplier must be float32 [n]")
    rowptr, col = _csr_idx(rowptr, col)
    dev = val.device
    mult = mult.contiguous()
    if csc is None:
        grad = torch.zeros(d, dtype=torch.float32, device=dev)  # accumulated
        rc = lib.agd_csr_grad_from_mult(
            _ptr(rowptr), _ptr(col), _ptr(val.contiguous()), _ptr(mult), n, d,
            _ptr(grad), None, None, None, 0, None, None, None, 0, 0, 1, None,
            None, _stream(val))
    else:
        grad = torch.empty(d, dtype=torch.float32, device=dev)  # overwritten
        cp, cr, cv = csc
        h = csc_heavy
        if h is not None and h["task_idx"].numel() > 0:
            heavy = (int(h["heavy_T"]), _ptr(h["cols"]), _ptr(h["taskptr"]),
                     _ptr(h["task_idx"]), h["cols"].numel(),
                     h["task_idx"].numel(), int(h["S"]), _ptr(h["partial"]),
                     _ptr(h.get("order")))
        else:
            heavy = (0, None, None, None, 0, 0, 1, None,
                     _ptr(h.get("order")) if h is not None else None)
        rc = lib.agd_csr_grad_from_mult(
            _ptr(rowptr), _ptr(col), _ptr(val.contiguous()), _ptr(mult), n, d,
            _ptr(grad), _ptr(cp), _ptr(cr), _ptr(cv), *heavy, _stream(val))
    _check(rc)
    return grad


# ---------------------------------------------------------------------------
# Column statistics / column scaling
# ---------------------------------------------------------------------------

def _colstats_out(d: int, dev):
    return (torch.empty(d, dtype=torch.float64, device=dev),
            torch.empty(d, dtype=torch.float64, device=dev),
            torch.empty(d, dtype=torch.float32, device=dev),
            torch.empty(d, dtype=torch.float32, device=dev),
            torch.empty(d, dtype=torch.int64, device=dev))


def _colstats_partials(m: int, dev):
    """Workspace for m partial records: (sum, sumsq) f64, (min, max) f32,
    nnz i32."""
    return (torch.empty(m, dtype=torch.float64, device=dev),
            torch.empty(m, dtype=torch.float64, device=dev),
            torch.empty(m, dtype=torch.float32, device=dev),
            torch.empty(m, dtype=torch.float32, device=dev),
            torch.empty(m, dtype=torch.int32, device=dev))


def dense_colstats(features: torch.Tensor):
    """(sum f64, sumsq f64, min f32, max f32, nnz i64), each [d], of a dense
    [n, d] shard in one pass (k_dense_colstats + k_colstats_reduce);
    bitwise reproducible."""
    lib = load()
    assert features.is_cuda and features.is_contiguous() and features.ndim == 2
    n, d = features.shape
    if n == 0 or d == 0:
        raise ValueError("dense_colstats needs a non-empty [n, d] matrix")
    a_dtype = _DTYPE_CODE[features.dtype]
    dev = features.device
    n_rb = int(lib.agd_colstats_rowblocks(n, d, a_dtype))
    part = _colstats_partials(n_rb * d, dev)
    out = _colstats_out(d, dev)
    rc = lib.agd_dense_colstats(
        _ptr(features), a_dtype, n, d, n_rb, *[_ptr(t) for t in part],
        *[_ptr(t) for t in out],
        int(os.environ.get("SPARKAGD_NT_LOADS", "1")), _stream(features))
    _check(rc)
    return out


def csr_colstats(csc, n: int, d: int, csc_heavy: Optional[dict] = None):
    """The dense_colstats tuple over the STORED entries of a CSC copy
    (colptr, row, val); empty columns report sum 0, min +inf, max -inf.
    Heavy columns go through the shard's task split when ``csc_heavy`` is
    given."""
    lib = load()
    colptr, _crow, cval = csc
    assert cval.is_cuda and cval.dtype == torch.float32
    if colptr.numel() != d + 1:
        raise ValueError("colptr must be [d + 1]")
    dev = cval.device
    out = _colstats_out(d, dev)
    if csc_heavy is not None and csc_heavy["task_idx"].numel() > 0:
        n_tasks = csc_heavy["task_idx"].numel()
        part = _colstats_partials(n_tasks, dev)
        rc = lib.agd_csc_colstats(
            _ptr(colptr), _ptr(cval), d, int(csc_heavy["heavy_T"]),
            _ptr(csc_heavy["cols"]), _ptr(csc_heavy["taskptr"]),
            _ptr(csc_heavy["task_idx"]), csc_heavy["cols"].numel(), n_tasks,
            int(csc_heavy["S"]), *[_ptr(t) for t in part],
            *[_ptr(t) for t in out], _stream(cval))
    else:
        rc = lib.agd_csc_colstats(
            _ptr(colptr), _ptr(cval), d, 2**31 - 1, None, None, None, 0, 0, 1,
            None, None, None, None, None, *[_ptr(t) for t in out],
            _stream(cval))
    _check(rc)
    return out


def dense_scale_cols(features: torch.Tensor, scale: torch.Tensor,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r, c] = features[r, c] * scale[c] in the features dtype (bf16/f32
    through an f32 product, f64 through f64); ``out`` may be ``features``."""
    lib = load()
    assert features.is_cuda and features.is_contiguous() and features.ndim == 2
    if features.dtype == torch.float8_e4m3fn:
        raise NotImplementedError(
            "fp8 features cannot be rescaled in place of their quantisation: "
            "scale the bf16/f32 data first, then quantise")
    n, d = features.shape
    if scale.numel() != d:
        raise ValueError("scale must be [d]")
    sdt = torch.float64 if features.dtype == torch.float64 else torch.float32
    scale = scale.to(device=features.device, dtype=sdt).contiguous()
    if out is None:
        out = torch.empty_like(features)
    elif (out.shape != features.shape or out.dtype != features.dtype
          or not out.is_contiguous() or out.device != features.device):
        raise ValueError("out must match features (shape, dtype, contiguous)")
    if n == 0 or d == 0:
        return out
    rc = lib.agd_dense_scale_cols(_ptr(features), _DTYPE_CODE[features.dtype],
                                  _ptr(scale), n, d, _ptr(out),
                                  _stream(features))
    _check(rc)
    if out is features:
        # written through its raw pointer: move the version counter so that
        # anything cached from the old values (DenseShard's packed copy) drops
        torch.autograd.graph.increment_version(out)
    return out


def _scale_vals_out(val: torch.Tensor, out: Optional[torch.Tensor]):
    assert val.is_cuda and val.dtype == torch.float32 and val.is_contiguous()
    if out is None:
        return torch.empty_like(val)
    if (out.shape != val.shape or out.dtype != val.dtype
            or not out.is_contiguous() or out.device != val.device):
        raise ValueError("out must match val (shape, dtype, contiguous)")
    return out


def csr_scale_vals(col: torch.Tensor, val: torch.Tensor, scale: torch.Tensor,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[k] = val[k] * scale[col[k]] (one f32 multiply)."""
    lib = load()
    out = _scale_vals_out(val, out)
    col = col.contiguous()
    if col.dtype != torch.int32:
        col = col.to(torch.int32)
    scale = scale.to(device=val.device, dtype=torch.float32).contiguous()
    rc = lib.agd_csr_scale_vals(_ptr(col), _ptr(val), _ptr(scale), val.numel(),
                                _ptr(out), _stream(val))
    _check(rc)
    return out


def csc_scale_vals(colptr: torch.Tensor, val: torch.Tensor,
                   scale: torch.Tensor, out: Optional[torch.Tensor] = None,
                   csc_heavy: Optional[dict] = None) -> torch.Tensor:
    """out[k] = val[k] * scale[c] for k in column c. Element-parallel with a
    colptr search, so no task split is needed; ``csc_heavy`` is accepted for
    symmetry with the other CSC entry points and not used."""
    lib = load()
    out = _scale_vals_out(val, out)
    colptr = colptr.contiguous()
    if colptr.dtype != torch.int32:
        colptr = colptr.to(torch.int32)
    d = colptr.numel() - 1
    if scale.numel() != d:
        raise ValueError("scale must be [d]")
    scale = scale.to(device=val.device, dtype=torch.float32).contiguous()
    rc = lib.agd_csc_scale_vals(_ptr(colptr), _ptr(val), _ptr(scale),
                                val.numel(), d, _ptr(out), _stream(val))
    _check(rc)
    return out


_cnt_ws_cache = {}


def _metrics_ws(device):
    """(int64 count partials, f64 sum partials) for the metrics kernels: one
    row per block, at most agd_metrics_max_blocks() rows of 6 / 7 words."""
    rows = int(load().agd_metrics_max_blocks())
    red = _red_ws(device)
    assert red.numel() >= rows * 7
    t = _cnt_ws_cache.get(device)
    if t is None:
        t = torch.empty(rows * 6, dtype=torch.int64, device=device)
        _cnt_ws_cache[device] = t
    return t, red


def _min_weight(bits: torch.Tensor, weighted: bool, n: int) -> torch.Tensor:
    """The kernels' min-weight word (sign-extended f32 bits) as an f32 0-dim."""
    if not weighted or n == 0:
        return torch.tensor(float("inf"), dtype=torch.float32,
                            device=bits.device)
    return bits.reshape(1).to(torch.int32).view(torch.float32)[0]


def binary_metrics(margins: torch.Tensor, labels: torch.Tensor,
                   edges: torch.Tensor, cut: float,
                   sample_weight: Optional[torch.Tensor] = None):
    """k_binary_metrics: (hist_pos, hist_neg, conf[4], sums f64[7], nan_count,
    min_weight) — see ``reference.binary_metrics`` for the contract."""
    lib = load()
    if margins.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"margins must be f32 or f64, got {margins.dtype}")
    z = margins.reshape(-1).contiguous()
    n = z.numel()
    dev = z.device
    edges = edges.to(device=dev, dtype=z.dtype).reshape(-1).contiguous()
    nbins = edges.numel() + 1
    from .reference import METRICS_MAX_BINS

    if nbins > METRICS_MAX_BINS:
        raise ValueError(f"at most {METRICS_MAX_BINS} bins, got {nbins}")
    labels = labels.to(device=dev, dtype=torch.float32).contiguous()
    sw = _prep_weights(sample_weight, dev)
    if labels.numel() != n or (sw is not None and sw.numel() != n):
        raise ValueError("labels / sample_weight must match margins [n]")
    ints = torch.zeros(2 * nbins + 6, dtype=torch.int64, device=dev)
    sums = torch.zeros(7, dtype=torch.float64, device=dev)
    cnt_ws, red_ws = _metrics_ws(dev)
    rc = lib.agd_binary_metrics(
        _ptr(z), _DTYPE_CODE[z.dtype], _ptr(labels), _ptr(sw), _ptr(edges),
        nbins, float(cut), n, _ptr(ints), _ptr(sums), _ptr(cnt_ws),
        _ptr(red_ws), _stream(z))
    _check(rc)
    b = nbins
    return (ints[:b], ints[b:2 * b], ints[2 * b:2 * b + 4], sums,
            ints[2 * b + 4], _min_weight(ints[2 * b + 5], sw is not None, n))


def multiclass_metrics(margins_padded_flat: torch.Tensor, labels: torch.Tensor,
                       k: int, kc: int,
                       sample_weight: Optional[torch.Tensor] = None):
    """k_multiclass_metrics: (conf [k, k], sums f64[2], bad_labels,
    min_weight) — see ``reference.multiclass_metrics``."""
    lib = load()
    z = margins_padded_flat.reshape(-1)
    if z.dtype != torch.float32:
        z = z.to(torch.float32)
    z = z.contiguous()
    if k < 2 or kc < k or z.numel() % kc:
        raise ValueError(f"bad class padding: k={k}, kc={kc}, {z.numel()} margins")
    n = z.numel() // kc
    dev = z.device
    labels = labels.to(device=dev, dtype=torch.float32).contiguous()
    sw = _prep_weights(sample_weight, dev)
    if labels.numel() != n or (sw is not None and sw.numel() != n):
        raise ValueError("labels / sample_weight must match margins [n]")
    ints = torch.zeros(k * k + 2, dtype=torch.int64, device=dev)
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    cnt_ws, red_ws = _metrics_ws(dev)
    rc = lib.agd_multiclass_metrics(
        _ptr(z), _ptr(labels), _ptr(sw), n, k, kc, _ptr(ints), _ptr(sums),
        _ptr(cnt_ws), _ptr(red_ws), _stream(z))
    _check(rc)
    return (ints[:k * k].reshape(k, k), sums, ints[k * k],
            _min_weight(ints[k * k + 1], sw is not None, n))
