"""Host-streamed shards: train on data larger than HBM.

The reference inherits Spark's cached-RDD spill/recompute path for data that
exceeds executor memory (SURVEY.md §5 'Failure detection' — implicit, free).
The MI355X-native analog: a shard whose features live in PINNED HOST MEMORY
and stream through a pair of device chunk buffers, with the H2D copies on a
dedicated HIP copy stream overlapped against the evaluation kernels on the
compute stream (double buffering: copy chunk i+1 while chunk i computes).

The evaluation is PCIe-bound by construction (~tens of GB/s vs the ~6.6 TB/s
HBM path), so this is a CAPACITY escape hatch — data up to host-RAM size per
GPU — not a speed path; the overlap keeps it at the copy ceiling instead of
copy+compute serialized. Labels, margins and the weight vector stay
device-resident, so margin-state tracking and the n-space multiplier work
exactly as for in-HBM shards.

Bytes over the host link are the only lever on this path, so a bf16 shard
can ``pack()`` itself into the lossless 12-bit format of ``packing.py``: the
host then holds (and every pass streams) 0.75x the bytes, and the packed
chunk kernels of the resident ``DenseShard`` consume the chunks directly.
``pack(release_raw=True)`` drops the raw host copy as well; whatever still
needs raw chunks gets them from the HIP decoder, bit for bit.

Binary losses only (the multiclass path dispatches on dense/CSR shard kinds).
On CPU the same code degrades to a plain chunked loop (tests/CI tier).
"""

from __future__ import annotations

import os
import time
from typing import Optional, Tuple

import torch

from . import ops, packing


class HostStreamedDenseShard:
    """Row-sharded dense design matrix in pinned host memory, streamed
    through device chunk buffers with copy/compute overlap."""

    kind = "dense_streamed"

    def __init__(
        self,
        features_host: torch.Tensor,
        labels: torch.Tensor,
        device: torch.device | str = "cuda",
        chunk_rows: int = 8192,
        sample_weight: Optional[torch.Tensor] = None,
    ):
        if features_host.ndim != 2:
            raise ValueError("features must be [n, d]")
        self.device = torch.device(device)
        self._cuda = self.device.type == "cuda"
        feats = features_host.contiguous()
        if self._cuda and not feats.is_pinned():
            feats = feats.pin_memory()
        self.features_host = feats
        self.labels = labels.to(self.device)
        if self.labels.dtype not in (torch.float32, torch.float64):
            self.labels = self.labels.to(torch.float32)
        self.sample_weight = None
        if sample_weight is not None:
            self.sample_weight = sample_weight.to(self.device, torch.float32)
        self.chunk_rows = int(chunk_rows)
        n, d = feats.shape
        self._n, self._d = int(n), int(d)
        self._dtype, self._elem_size = feats.dtype, feats.element_size()
        if self._cuda:
            self._buf = [
                torch.empty((min(self.chunk_rows, self._n), d),
                            dtype=feats.dtype, device=self.device)
                for _ in range(2)
            ]
            self._copy_stream = torch.cuda.Stream(self.device)
            self._fence_copy_stream()
            self._copy_done = [torch.cuda.Event(), torch.cuda.Event()]
            self._compute_done = [torch.cuda.Event(), torch.cuda.Event()]
        # 12-bit packed host copy (packing.py): [n, pack_row_bytes(d)] uint8,
        # one table for the shard, escape side lists per chunk (device)
        self._packed_host: Optional[torch.Tensor] = None
        self._packed_key = None
        self._pack_table = None
        self._pack_esc: list = []     # per chunk: (esc dict, nnz)
        self._pack_nnz = 0
        self._pbuf = None             # device chunk buffers of packed bytes
        #: why the last pack() was refused (None after a successful one)
        self.pack_refused: Optional[str] = None
        #: wall time of the last successful pack()
        self.pack_seconds: Optional[float] = None

    # --- shard interface ---

    @property
    def n(self) -> int:
        return self._n

    @property
    def d(self) -> int:
        return self._d

    @property
    def feature_dtype(self) -> torch.dtype:
        """dtype of the logical features (valid with the raw copy released)."""
        return self._dtype

    @property
    def nbytes(self) -> int:
        """Logical raw size, packed or not (as ``DenseShard.nbytes``)."""
        return self._n * self._d * self._elem_size

    @property
    def streamed_nbytes(self) -> int:
        """Bytes one feature pass moves host-to-device."""
        if self.is_packed:
            return self._packed_host.numel()
        return self.nbytes

    def _fence_copy_stream(self) -> None:
        """Order the copy stream after everything queued so far on the
        current stream. A fresh chunk buffer may be a block that the caching
        allocator just took back from a tensor whose last kernel is still
        queued there; the first H2D copy into it runs on the copy stream and
        has no other reason to wait for that kernel."""
        self._copy_stream.wait_stream(torch.cuda.current_stream(self.device))

    def _chunks(self):
        for lo in range(0, self._n, self.chunk_rows):
            yield lo, min(lo + self.chunk_rows, self._n)

    def _stream_chunks(self, host: torch.Tensor, bufs, fn) -> None:
        """Run ``fn(chunk_on_device, i, lo, hi)`` over the row chunks of the
        host tensor ``host`` (the raw features or the packed bytes) through
        the device buffer pair ``bufs``, with double-buffered H2D copies
        overlapping the compute stream. The events are shared by both buffer
        pairs: chunk i of any pass waits for the last compute that used
        slot i % 2, whichever pair it read."""
        main = torch.cuda.current_stream(self.device)
        for i, (lo, hi) in enumerate(self._chunks()):
            b = i % 2
            buf = bufs[b][: hi - lo]
            with torch.cuda.stream(self._copy_stream):
                # Buffer reuse: wait for the LAST compute that read this
                # buffer — chunk i-2 of this pass, or (for i < 2) the tail
                # chunks of the PREVIOUS pass, whose events persist across
                # calls. Waiting unconditionally covers back-to-back passes
                # with no intervening host sync (an event never recorded is
                # a no-op wait).
                self._copy_stream.wait_event(self._compute_done[b])
                buf.copy_(host[lo:hi], non_blocking=True)
                self._copy_done[b].record(self._copy_stream)
            main.wait_event(self._copy_done[b])
            fn(buf, i, lo, hi)
            self._compute_done[b].record(main)

    def _for_each_chunk(self, fn) -> None:
        """Run ``fn(chunk_features_device, lo, hi)`` over all chunks in the
        features' own dtype: streamed from the raw host copy, or, once that
        is released, from the packed copy through the decoder."""
        if self.features_host is None:
            self._for_each_decoded_chunk(fn)
        elif not self._cuda:
            for lo, hi in self._chunks():
                fn(self.features_host[lo:hi], lo, hi)
        else:
            self._stream_chunks(self.features_host, self._buf,
                                lambda buf, i, lo, hi: fn(buf, lo, hi))

    def _for_each_packed_chunk(self, fn) -> None:
        """Run ``fn(PackedDense view of the chunk, lo, hi)`` over all chunks
        of the packed copy (device shards)."""
        self._stream_chunks(
            self._packed_host, self._pbuf,
            lambda pbuf, i, lo, hi: fn(self._chunk_view(pbuf, i, lo, hi), lo, hi))

    def _for_each_decoded_chunk(self, fn) -> None:
        """Run ``fn(bf16 chunk, lo, hi)`` from the packed copy: the packed
        chunk crosses the link and is decoded into the raw chunk buffer."""
        if not self._cuda:
            for i, (lo, hi) in enumerate(self._chunks()):
                pk = self._chunk_view(self._packed_host[lo:hi], i, lo, hi)
                fn(ops.dense_pack_decode(pk), lo, hi)
            return

        def step(pbuf, i, lo, hi):
            pk = self._chunk_view(pbuf, i, lo, hi)
            fn(ops.dense_pack_decode(pk, out=self._buf[i % 2][: hi - lo]), lo, hi)

        self._stream_chunks(self._packed_host, self._pbuf, step)

    def _chunk_view(self, packed_chunk: torch.Tensor, i: int, lo: int, hi: int):
        esc, nnz = self._pack_esc[i]
        return packing.PackedDense(packed_chunk, self._pack_table, hi - lo,
                                   self._d, esc, nnz, 0.0)

    # --- 12-bit packed copy ---

    def _features_key(self):
        f = self.features_host
        return (f.data_ptr(), tuple(f.shape), f.dtype, f._version)

    @property
    def is_packed(self) -> bool:
        """True while a packed copy is held that still matches the raw host
        copy; an in-place change of ``features_host`` drops it."""
        if (self._packed_host is not None and self.features_host is not None
                and self._packed_key != self._features_key()):
            self._drop_packed()
        return self._packed_host is not None

    @property
    def streams_packed_on_gpu(self) -> bool:
        """Whether the packed chunk kernels can serve this shard."""
        return self._cuda and os.environ.get("SPARKAGD_FORCE_REFERENCE") != "1"

    def _drop_packed(self) -> None:
        self._packed_host = None
        self._packed_key = None
        self._pack_table = None
        self._pack_esc = []
        self._pack_nnz = 0
        self._pbuf = None

    def pack(self, release_raw: bool = False) -> bool:
        """Build (or keep) the lossless 12-bit packed host copy of a bf16
        shard; every pass then streams 0.75x the bytes. Two passes over the
        raw chunks: the high-byte histogram (one table for the whole shard),
        then the encode, chunk by chunk, into one pinned uint8 tensor, with
        the escape side lists kept per chunk on the device. Returns False,
        with the reason in ``pack_refused`` and the shard still streaming
        raw, when it cannot be packed. ``release_raw=True`` drops
        ``features_host`` once the packed copy is complete (host RAM is this
        shard kind's limit); ``unpack()`` rebuilds it."""
        if not self.is_packed:
            self.pack_refused = self._build_packed()
            if self.pack_refused is not None:
                return False
        if release_raw:
            self.features_host = None
            self._packed_key = None
        return True

    def _build_packed(self) -> Optional[str]:
        """Pack from the raw host copy; the refusal reason, or None."""
        feats = self.features_host
        n, d = self._n, self._d
        why = packing.pack_refusal(feats)
        if why is not None:
            return why
        row_bytes = packing.pack_row_bytes(d)
        if row_bytes >= 2 * d:
            return (f"a packed row ({row_bytes} B, padded to 384 B) is not "
                    f"smaller than the raw row ({2 * d} B)")
        t0 = time.perf_counter()
        # pass 1: per-chunk histograms, summed as integers on the host
        chunk_hist = []
        self._for_each_chunk(
            lambda buf, lo, hi: chunk_hist.append(packing._hist(buf)))
        table, n_esc = packing.choose_pack_table(
            torch.stack(chunk_hist).sum(0).tolist())
        why = packing.escape_cap_refusal(n_esc, n, d)
        if why is not None:
            return why
        chunk_esc = [int(h.sum()) - sum(int(h[v]) for v in table)
                     for h in chunk_hist]
        chunk_cap = min(self.chunk_rows, n)
        if self._cuda:
            side = 16 * n_esc + sum(
                (chunk_cap + d + 2) * 4 for e in chunk_esc if e > 0)
            need = side + 2 * chunk_cap * row_bytes
            free, _total = torch.cuda.mem_get_info(self.device)
            if free - need < packing.PACK_HEADROOM_BYTES:
                return (f"side lists and packed chunk buffers ({need} B) would "
                        f"not leave {packing.PACK_HEADROOM_BYTES} B of device "
                        f"memory free")
        packed_host = torch.empty((n, row_bytes), dtype=torch.uint8,
                                  pin_memory=self._cuda)
        side_lists = []

        # pass 2: encode each chunk; the D2H copy is queued on the compute
        # stream, after its encode and before the chunk loop lets the copy
        # stream reuse the staging buffer
        def encode(buf, lo, hi):
            nnz = chunk_esc[len(side_lists)]
            packed, esc = packing.encode_with_table(buf, table, nnz)
            packed_host[lo:hi].copy_(packed, non_blocking=True)
            side_lists.append((esc, nnz))

        self._for_each_chunk(encode)
        if self._cuda:
            torch.cuda.synchronize(self.device)  # also quiesces reused blocks
            self._pbuf = [torch.empty((chunk_cap, row_bytes), dtype=torch.uint8,
                                      device=self.device) for _ in range(2)]
        self._packed_host = packed_host
        self._pack_table = table
        self._pack_esc = side_lists
        self._pack_nnz = n_esc
        self._packed_key = self._features_key()
        self.pack_seconds = time.perf_counter() - t0
        return None

    def unpack(self) -> None:
        """Drop the packed copy (the shard streams the raw features again).
        With the raw copy released, it is first rebuilt from the packed one,
        bit for bit: decode per chunk, then D2H into a pinned tensor."""
        if self._packed_host is None:
            return
        if self.features_host is None:
            raw = torch.empty((self._n, self._d), dtype=self._dtype,
                              pin_memory=self._cuda)
            self._for_each_decoded_chunk(
                lambda buf, lo, hi: raw[lo:hi].copy_(buf, non_blocking=True))
            if self._cuda:
                torch.cuda.synchronize(self.device)
            self.features_host = raw
        self._drop_packed()

    def _packed_route(self, vec: torch.Tensor) -> bool:
        """Whether a pass with the n- or d-vector ``vec`` reads the packed
        copy. The packed kernels take f32 vectors (as on a packed
        DenseShard): another dtype streams raw while the raw copy is held."""
        if not self.is_packed:
            return False
        if not self.streams_packed_on_gpu:
            # no packed kernel off the GPU: decoded chunks, ordinary ops
            return True
        if vec.dtype == torch.float32 or self.features_host is None:
            return True   # a non-f32 vector raises in the packed op
        return False

    def _slice(self, t: Optional[torch.Tensor], lo: int, hi: int):
        return None if t is None else t[lo:hi]

    def eval(self, w: torch.Tensor, loss_type: int,
             mask: Optional[torch.Tensor] = None, need_grad: bool = True
             ) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
        grad = None
        loss_count = torch.zeros(2, dtype=torch.float64, device=self.device)
        packed = self._packed_route(w) and self.streams_packed_on_gpu

        def step(buf, lo, hi):
            nonlocal grad
            op = ops.dense_eval_packed if packed else ops.dense_eval
            g, lc = op(buf, self.labels[lo:hi], w, loss_type,
                       self._slice(mask, lo, hi), need_grad,
                       self._slice(self.sample_weight, lo, hi))
            loss_count.add_(lc)
            if need_grad:
                grad = g if grad is None else ops.axpby(1.0, grad, 1.0, g)

        self._run_pass(step, w)
        return grad, loss_count

    def _run_pass(self, step, vec: torch.Tensor) -> None:
        """One feature pass: ``step`` gets PackedDense chunk views on the
        packed GPU route, decoded bf16 chunks on the packed route elsewhere,
        raw chunks otherwise."""
        if not self._packed_route(vec):
            self._for_each_chunk(step)
        elif self.streams_packed_on_gpu:
            self._for_each_packed_chunk(step)
        else:
            self._for_each_decoded_chunk(step)

    def margins(self, v: torch.Tensor) -> torch.Tensor:
        out = torch.empty(self._n, dtype=v.dtype, device=self.device)
        packed = self._packed_route(v) and self.streams_packed_on_gpu

        def step(buf, lo, hi):
            op = ops.dense_margins_packed if packed else ops.dense_margins
            out[lo:hi] = op(buf, v)

        self._run_pass(step, v)
        return out

    def eval_from_margins(self, margins: torch.Tensor, loss_type: int,
                          mask: Optional[torch.Tensor] = None,
                          need_grad: bool = True):
        # The multiplier stage is n-space elementwise (no feature pass);
        # the torch formulation runs on the device margins directly.
        mult, loss = ops.reference._multiplier_and_loss(margins, self.labels,
                                                        loss_type)
        mult, loss, count = ops.reference._apply_mask_weight(
            mult, loss, mask, self.sample_weight, self._n, self.device)
        loss_count = torch.stack([loss.to(torch.float64).sum(), count])
        if not need_grad:
            return None, loss_count
        grad = None
        packed = self._packed_route(mult) and self.streams_packed_on_gpu
        if packed and mult.dtype != torch.float32:
            raise TypeError(f"multiplier dtype {mult.dtype} must be "
                            f"torch.float32 for a packed bf16 shard")

        def step(buf, lo, hi):
            nonlocal grad
            op = (ops.dense_grad_from_mult_packed if packed
                  else ops.dense_grad_from_mult)
            g = op(buf, mult[lo:hi].contiguous())
            grad = g if grad is None else ops.axpby(1.0, grad, 1.0, g)

        self._run_pass(step, mult)
        return grad, loss_count
