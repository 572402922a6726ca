"""Lossless 12-bit packed copy of a bf16 dense shard.

A bf16 value is 1 sign bit, 8 exponent bits and 7 mantissa bits, and in real
feature data the high seven exponent bits take very few distinct values. The
packed copy stores, per element, the low byte (``e0 | m6..m0``) raw plus a
4-bit code ``s<<3 | k`` where ``k`` indexes an 8-entry table of high-byte
magnitudes (``e7..e1``). Eight adjacent elements of a row form one 12-byte
group: dwords 0 and 1 hold the low bytes of elements 0-3 and 4-7, dword 2
holds the eight codes (byte ``j``: element ``j`` in the low nibble, element
``4+j`` in the high nibble). A row is padded with zero groups to a multiple
of 32 groups (384 bytes), which keeps every wave's sweep on 128-byte lines.
The stream kernels decode a group with ten byte permutes and read 0.75x the
bytes of the raw shard.

Table slot 0 is always ``0x00``: elements whose high-byte magnitude is not in
the table ("escapes") are stored as the all-zero code, decode to ``+0.0`` and
carry their true value in a sparse side list (row-sorted for ``A·v``,
column-sorted for ``Aᵀ·m``) that small correction kernels add back. A shard
whose escapes exceed ``PACK_ESCAPE_CAP`` of its elements is not packed.

The format, the decode and the measured figures are in ``docs/KERNELS.md``.
"""

from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

import torch

#: escapes above this fraction of the elements refuse the pack: at 2^-10 the
#: side lists (8 B + a gathered line per escape) already eat about a seventh
#: of the 0.5 B/element the packed stream saves
PACK_ESCAPE_CAP = 2.0 ** -10

#: ``pack_dense="auto"`` packs only shards that cannot sit in the 256 MB
#: Infinity Cache (a cached shard is not HBM-bound)
PACK_MIN_BYTES = 256 << 20

#: iterations after which the one-time pack has paid for itself. ``auto``
#: packs before iteration 1 of a solve, normally the first pack of the
#: process, so the gate is the cold figure: measured on MI355X at
#: 16384 x 10^6 the first pack of a process takes 77-84 ms and an iteration
#: saves 2.43 ms, 32-35 iterations, rounded up
#: (profiles/pack_stream_tails.log). A later pack in the same process takes
#: 19 ms (8 iterations).
PACK_BREAK_EVEN_ITERS = 35

#: device memory that must stay free after the 0.75x copy is allocated
PACK_HEADROOM_BYTES = 8 << 30


def choose_pack_table(hist: Sequence[int]) -> Tuple[List[int], int]:
    """Pick the 8-entry high-byte table from a 128-bin histogram.

    The 8 most frequent magnitudes, ties broken by the lower value; if
    ``0x00`` is not among them it replaces the least frequent of the eight
    (a 7+zero table), because slot 0 must decode escapes to ``+0.0``. The
    table is returned in ascending order, so slot 0 is ``0x00``. Also
    returns the number of escapes the table leaves.
    """
    counts = [int(c) for c in hist]
    if len(counts) != 128:
        raise ValueError("histogram must have 128 bins")
    ranked = sorted(range(128), key=lambda v: (-counts[v], v))
    top = ranked[:8]
    if 0 not in top:
        top = top[:7] + [0]
    table = sorted(top)
    escapes = sum(counts) - sum(counts[v] for v in table)
    return table, escapes


def table_luts(table: Sequence[int]) -> Tuple[int, int]:
    """The table as the two u32 kernel arguments (slots 0-3, slots 4-7)."""
    if len(table) != 8 or table[0] != 0 or any(not 0 <= t < 128 for t in table):
        raise ValueError("table must be 8 magnitudes in [0, 128) with slot 0 == 0")
    lo = sum(int(t) << (8 * i) for i, t in enumerate(table[:4]))
    hi = sum(int(t) << (8 * i) for i, t in enumerate(table[4:]))
    return lo, hi


class PackedDense:
    """The packed copy of one bf16 shard plus its escape side lists."""

    def __init__(self, packed: torch.Tensor, table: List[int], n: int, d: int,
                 esc: dict, nnz: int, seconds: float):
        self.packed = packed          # [n, pack_row_bytes(d)] uint8
        self.table = list(table)
        self.lut_lo, self.lut_hi = table_luts(table)
        self.n, self.d = n, d
        self.esc = esc                # rowptr/col/val (CSR), colptr/row/cval (CSC)
        self.nnz = nnz
        self.seconds = seconds        # wall time of the pack

    @property
    def nbytes(self) -> int:
        side = sum(t.numel() * t.element_size() for t in self.esc.values()
                   if t is not None)
        return self.packed.numel() + side


def pack_row_bytes(d: int) -> int:
    """Bytes of one packed row: d/8 groups of 12 B, padded to 32 groups."""
    return (d // 8 + 31) // 32 * 32 * 12


def _hist(features: torch.Tensor) -> torch.Tensor:
    from . import ops

    if ops._use_hip(features):
        return ops._get_hip().dense_pack_hist(features)
    h = (features.view(torch.int16).to(torch.int32) >> 8) & 0x7F
    return torch.bincount(h.reshape(-1).cpu(), minlength=128)


def _encode_torch(features: torch.Tensor, table: Sequence[int]):
    """Plain-torch encoder (CPU shards; the format's reference)."""
    n, d = features.shape
    u = features.view(torch.int16).to(torch.int32) & 0xFFFF
    slot_of = torch.full((128,), -1, dtype=torch.int32, device=u.device)
    slot_of[torch.as_tensor(list(table), device=u.device)] = torch.arange(
        8, dtype=torch.int32, device=u.device)
    slot = slot_of[((u >> 8) & 0x7F).long()]
    esc = slot < 0
    zero = torch.zeros_like(u)
    code = torch.where(esc, zero, ((u >> 15) << 3) | slot).view(n, d // 8, 8)
    low = torch.where(esc, zero, u & 0xFF).view(n, d // 8, 8)
    out = torch.zeros((n, pack_row_bytes(d) // 12, 12), dtype=torch.uint8,
                      device=u.device)
    out[:, :d // 8, 0:8] = low.to(torch.uint8)
    out[:, :d // 8, 8:12] = (code[..., 0:4] | (code[..., 4:8] << 4)).to(torch.uint8)
    return out.view(n, pack_row_bytes(d)), esc


def _no_escapes() -> dict:
    return {k: None for k in ("rowptr", "col", "val", "colptr", "row", "cval")}


def pack_refusal(features: torch.Tensor) -> Optional[str]:
    """Why this tensor cannot be packed at all (shape/dtype), or None."""
    if features.dtype != torch.bfloat16:
        return f"dtype {features.dtype} (bf16 only)"
    if features.ndim != 2 or features.shape[0] < 1 or features.shape[1] < 8:
        return "needs an [n >= 1, d >= 8] matrix"
    if features.shape[1] % 8 != 0:
        return f"d = {features.shape[1]} is not a multiple of 8"
    if not features.is_contiguous():
        return "features are not row-major contiguous"
    if features.data_ptr() % 16 != 0:
        return "features are not 16-byte aligned"
    return None


def encode_with_table(features: torch.Tensor, table: Sequence[int],
                      n_esc: int) -> Tuple[torch.Tensor, dict]:
    """The table-given half of a pack: the packed bytes of ``features`` (a
    whole shard, or one chunk of a streamed one) under ``table`` and the
    escape side lists, rows local to ``features``. ``n_esc`` is the number of
    elements whose high byte is not in the table (known from the histogram).
    Work is queued on the current stream; the caller synchronises."""
    from . import ops

    n, d = features.shape
    esc = _no_escapes()
    if ops._use_hip(features):
        hip = ops._get_hip()
        lo, hi = table_luts(table)
        packed, esc_count, flags = hip.dense_pack_encode(features, lo, hi)
        if n_esc > 0:
            dev = features.device
            rowptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
            torch.cumsum(esc_count, 0, dtype=torch.int32, out=rowptr[1:])
            col, val = hip.dense_pack_escapes(features, lo, hi, flags, rowptr,
                                              n_esc)
            rows = torch.repeat_interleave(
                torch.arange(n, dtype=torch.int32, device=dev),
                esc_count.long(), output_size=n_esc)
            order = torch.sort(col.long(), stable=True).indices
            colptr = torch.zeros(d + 1, dtype=torch.int32, device=dev)
            torch.cumsum(torch.bincount(col.long(), minlength=d), 0,
                         dtype=torch.int32, out=colptr[1:])
            esc = {"rowptr": rowptr, "col": col, "val": val, "colptr": colptr,
                   "row": rows[order].contiguous(), "cval": val[order].contiguous()}
        del flags
    else:
        packed, esc_mask = _encode_torch(features, table)
        if n_esc > 0:
            rows, cols = esc_mask.nonzero(as_tuple=True)
            val = features[rows, cols].to(torch.float32)
            rowptr = torch.zeros(n + 1, dtype=torch.int32, device=rows.device)
            rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
            order = torch.sort(cols, stable=True).indices
            colptr = torch.zeros(d + 1, dtype=torch.int32, device=rows.device)
            colptr[1:] = torch.cumsum(torch.bincount(cols, minlength=d), 0)
            esc = {"rowptr": rowptr, "col": cols.to(torch.int32), "val": val,
                   "colptr": colptr, "row": rows[order].to(torch.int32),
                   "cval": val[order]}
    return packed, esc


def escape_cap_refusal(n_esc: int, n: int, d: int) -> Optional[str]:
    """The refusal reason when ``n_esc`` escapes exceed the cap, or None."""
    if n_esc > PACK_ESCAPE_CAP * n * d:
        return (f"escape fraction {n_esc / (n * d):.3e} exceeds "
                f"{PACK_ESCAPE_CAP:.3e}")
    return None


def pack_features(features: torch.Tensor) -> Tuple[Optional[PackedDense], Optional[str]]:
    """Build the packed copy; returns ``(None, reason)`` when refused."""
    import time

    why = pack_refusal(features)
    if why is not None:
        return None, why
    t0 = time.perf_counter()
    n, d = features.shape
    table, n_esc = choose_pack_table(_hist(features).tolist())
    why = escape_cap_refusal(n_esc, n, d)
    if why is not None:
        return None, why
    packed, esc = encode_with_table(features, table, n_esc)
    if features.is_cuda:
        torch.cuda.synchronize(features.device)
    return PackedDense(packed, table, n, d, esc, n_esc,
                       time.perf_counter() - t0), None


def decode_torch(packed: torch.Tensor, table: Sequence[int], d: int,
                 esc: Optional[dict] = None) -> torch.Tensor:
    """Plain-torch decoder: packed ``[n, pack_row_bytes(d)]`` uint8 back to
    the bf16 ``[n, d]`` matrix, bit for bit, with the escapes of the CSR side
    list ``esc`` (``rowptr/col/val``) scattered back in. Integer moves only,
    so NaN payloads, infinities and -0.0 survive."""
    n = packed.shape[0]
    p = packed.view(n, -1, 12)[:, :d // 8].to(torch.int32)
    tab = torch.as_tensor(list(table), dtype=torch.int32, device=packed.device)
    bits = torch.empty((n, d // 8, 8), dtype=torch.int32, device=packed.device)
    for k in range(8):
        code = (p[:, :, 8 + (k & 3)] >> (4 * (k >> 2))) & 0xF
        high = tab[(code & 7).long()] | ((code >> 3) << 7)
        bits[:, :, k] = (high << 8) | p[:, :, k]
    bits = bits.view(n, d)
    if esc is not None and esc.get("col") is not None and esc["col"].numel():
        counts = torch.diff(esc["rowptr"].long())
        rows = torch.repeat_interleave(
            torch.arange(n, device=packed.device), counts)
        bits[rows, esc["col"].long()] = \
            (esc["val"].view(torch.int32) >> 16) & 0xFFFF
    # two's-complement wrap of the 16-bit pattern into int16, then reinterpret
    return bits.to(torch.int16).view(torch.bfloat16)


def auto_pack_wanted(features: torch.Tensor, planned_iterations: int) -> bool:
    """The cheap part of the ``pack_dense="auto"`` decision (everything but
    the escape count, which ``pack_features`` checks itself)."""
    if not features.is_cuda or pack_refusal(features) is not None:
        return False
    if os.environ.get("SPARKAGD_FORCE_REFERENCE") == "1":
        return False
    raw = features.numel() * 2
    if raw <= PACK_MIN_BYTES:
        return False
    if planned_iterations < PACK_BREAK_EVEN_ITERS:
        return False
    free, _total = torch.cuda.mem_get_info(features.device)
    return free >= raw * 3 // 4 + PACK_HEADROOM_BYTES


def _dense_parts(data):
    kind = getattr(data, "kind", None)
    if kind == "dense":
        return [data]
    if kind == "intercept":
        return _dense_parts(data.inner)
    if kind == "mixed":
        return [p for part in data.parts for p in _dense_parts(part)]
    return []


def gradient_streams_shard(gradient) -> bool:
    """True when the gradient evaluates through the shard's own ``eval`` /
    ``margins`` / ``eval_from_margins``, the only consumers of a packed
    copy. The multiclass gradient (and any subclass that overrides those
    methods) hands ``shard.features`` to its own kernels, so a copy would
    only cost memory; an object that cannot be identified counts as such.
    Wrappers are followed through their ``inner`` attribute."""
    from .models.gradient import Gradient

    g = gradient
    for _ in range(8):
        if isinstance(g, Gradient) or not hasattr(g, "inner"):
            break
        g = g.inner
    if not isinstance(g, Gradient) or getattr(g, "IS_MULTICLASS", False):
        return False
    return all(getattr(type(g), name) is getattr(Gradient, name)
               for name in ("eval", "margins", "eval_from_margins"))


def apply_pack_policy(data, pack_dense, planned_iterations: int,
                      gradient=None) -> None:
    """``run()``'s ``pack_dense`` knob applied to every dense shard reachable
    from ``data`` (the shard itself, the inner shard of an InterceptShard,
    the dense parts of a MixedShard). Nothing is packed, under ``"auto"`` or
    ``True``, for a ``gradient`` that does not stream through the shard's
    routed methods. A refused pack leaves the shard on the raw path and its
    reason in ``pack_refused``.

    A host-streamed shard on a GPU is packed under ``True`` only (its bytes
    then cross the host link at 0.75x); ``"auto"`` leaves it raw, because
    its break-even against the one-time pack is not part of the gate yet."""
    if pack_dense is False:
        return
    if gradient is not None and not gradient_streams_shard(gradient):
        return
    if getattr(data, "kind", None) == "dense_streamed":
        if pack_dense is True and data.streams_packed_on_gpu and not data.is_packed:
            data.pack()
        return
    for shard in _dense_parts(data):
        if shard.is_packed:
            continue
        if pack_dense is True:
            if shard.features.is_cuda:
                shard.pack()
        elif auto_pack_wanted(shard.features, planned_iterations):
            shard.pack()
