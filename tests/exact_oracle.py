"""Test data on which f32 arithmetic is exact, and its f64 oracle.

Features, weights and multipliers are small integers (entries in {-2..2},
many zero). They are exact in bf16, f32, f64 and float8_e4m3fn, and every
product and every partial sum is an integer below 2^24, so ANY summation
order, fma contraction, slab / row-block split or float atomic gives the one
exact result. A kernel output is therefore compared with ``torch.equal``
against the f64 oracle cast to the kernel's accumulator dtype
(:func:`exact_equal`): no tolerance, at any ``d``.

For least squares (``m = 2(z-y)``, ``l = (z-y)^2``) and hinge
(``m in {-s, 0}``, ``l = 1 - s*z``) the multiplier, the loss, the f64 loss sum
and the gradient stay exact too, also under dyadic sample weights
{0.5, 1, 2}. The generators check the ranges they rely on (``_check_range``).

Everything is generated on the CPU from a seed and cached: tests share one
copy and must not modify it.
"""

from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch

LSQ, HINGE = 1, 2  # ops.LOSS_LEAST_SQUARES / ops.LOSS_HINGE

DTYPES = {
    "bf16": torch.bfloat16,
    "f32": torch.float32,
    "f64": torch.float64,
    "fp8": torch.float8_e4m3fn,
}
#: elements per 16-byte lane load (the kernels' W) and rows per margins group
W_FULL = {"bf16": 8, "f32": 4, "f64": 2, "fp8": 16}
ROWS = {"bf16": 4, "f32": 4, "f64": 4, "fp8": 8}
DTYPE_CODE = {"bf16": 0, "f32": 1, "f64": 2, "fp8": 3}

EXACT_LIMIT = float(2 ** 24)


def acc_dtype(name: str) -> torch.dtype:
    return torch.float64 if name == "f64" else torch.float32


def exact_equal(got: torch.Tensor, oracle64: torch.Tensor) -> bool:
    """THE comparison of the exact tests: ``got`` (a kernel's output, any
    device) equals the f64 oracle cast to ``got``'s dtype, bit for bit as
    numbers (``torch.equal``: same shape, no tolerance, NaN never equal)."""
    assert oracle64.dtype == torch.float64
    g = got.detach().cpu()
    return g.shape == oracle64.shape and torch.equal(g, oracle64.cpu().to(g.dtype))


def _gen(seed: int) -> torch.Generator:
    return torch.Generator(device="cpu").manual_seed(seed)


def _ints(shape, g, p_zero=0.5) -> torch.Tensor:
    """f64 tensor of integers in {-2..2}, zero with probability ``p_zero``."""
    v = torch.randint(1, 3, shape, generator=g).double()
    v = v * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)
    return v * (torch.rand(shape, generator=g) >= p_zero).double()


def _nonzero_ints(shape, g) -> torch.Tensor:
    return _ints(shape, g, p_zero=0.0)


def _labels_for(z: torch.Tensor, g, flip_interior: bool) -> torch.Tensor:
    """y = [z <= 0]: then z - y != 0 and s*z <= 0 < 1, so neither loss has a
    zero multiplier. ``flip_interior`` flips a quarter of the rows that are
    away from both ends and have |z| >= 2: least squares stays non-zero,
    hinge gets inactive rows (m = 0, l = 0) away from the tails."""
    y = (z <= 0).double()
    n = z.numel()
    if flip_interior and n > 16:
        flip = (torch.rand(n, generator=g) < 0.25) & (z.abs() >= 2)
        flip[:8] = False
        flip[-8:] = False
        y = torch.where(flip, 1.0 - y, y)
    return y


def _check_range(absz, abs_grad_terms=None):
    """Every partial sum is bounded by the sum of absolute terms."""
    if absz.numel():
        assert float(absz.max()) + 1 < 4096, "need |z - y| < 4096"
    if abs_grad_terms is not None and abs_grad_terms.numel():
        assert float(abs_grad_terms.max()) < EXACT_LIMIT


# --------------------------------------------------------------------------
# losses in f64
# --------------------------------------------------------------------------

def mult_loss64(z: torch.Tensor, y: torch.Tensor, loss_type: int):
    """(m, l) per example in f64 for least squares and hinge."""
    if loss_type == LSQ:
        diff = z - y
        return 2.0 * diff, diff * diff
    assert loss_type == HINGE
    s = 2.0 * y - 1.0
    sz = s * z
    act = sz < 1.0
    zero = torch.zeros_like(z)
    return torch.where(act, -s, zero), torch.where(act, 1.0 - sz, zero)


def apply_mask_weight64(m, l, n, mask=None, sw=None):
    """(m, l, count) after the mask and the sample weights; masked rows do
    not enter the count, which is the unmasked weight sum."""
    keep = torch.ones(n, dtype=torch.float64) if mask is None else mask.double()
    wts = torch.ones(n, dtype=torch.float64) if sw is None else sw.double()
    # where(), not a product: a masked row may carry a non-finite margin
    zero = torch.zeros_like(m)
    m = torch.where(keep > 0, m * wts, zero)
    l = torch.where(keep > 0, l * wts, zero)
    return m, l, (keep * wts).sum()


def grad64(A64: torch.Tensor, m64: torch.Tensor) -> torch.Tensor:
    """A^T m over the rows with m != 0 only (the kernels' skip contract: a
    row whose multiplier is exactly 0 is never read, whatever it holds)."""
    rows = torch.nonzero(m64 != 0).reshape(-1)
    return A64[rows].T @ m64[rows]


def dense_eval64(p, loss_type, mask=None, sw=None, z=None):
    """(grad f64 [d], loss_count f64 [2], mult f64 [n]) of a dense problem."""
    z = p.z64 if z is None else z
    m, l = mult_loss64(z, p.y64, loss_type)
    m, l, cnt = apply_mask_weight64(m, l, p.n, mask, sw)
    _check_range(torch.zeros(1), p.A64.nan_to_num(0, 0, 0).abs().T @ m.abs())
    return grad64(p.A64, m), torch.stack([l.sum(), cnt]), m


# --------------------------------------------------------------------------
# dense problems
# --------------------------------------------------------------------------

@functools.lru_cache(maxsize=128)
def dense_problem(n: int, d: int, dtype_name: str, seed: int = 0,
                  w_nnz: int = 16):
    """A [n, d] in ``dtype_name``, w [d] and labels with the generator rules:
    the first and last row and the first and last column are non-zero
    everywhere and meet non-zero w entries; w has at most ``w_nnz`` + 2
    non-zeros (so |z| stays small); labels from :func:`_labels_for`."""
    g = _gen(1000003 * seed + 7919 * n + d)
    A64 = _ints((n, d), g)
    for idx in ((0, slice(None)), (n - 1, slice(None)),
                (slice(None), 0), (slice(None), d - 1)):
        A64[idx] = _nonzero_ints(A64[idx].shape, g)
    w64 = torch.zeros(d, dtype=torch.float64)
    pick = torch.randint(0, d, (w_nnz,), generator=g)
    w64[pick] = _nonzero_ints((w_nnz,), g)
    w64[0], w64[d - 1] = 2.0, -1.0
    if d > 1:
        w64[d - 2] = 1.0  # the column before the last: a W-tail of length 2
    z64 = A64 @ w64
    y64 = _labels_for(z64, g, flip_interior=True)
    _check_range(A64.abs() @ w64.abs())
    # multipliers for the raw A^T m path: non-zero integers
    m64 = _nonzero_ints((n,), g)
    _check_range(torch.zeros(1), A64.abs().T @ m64.abs())
    sw = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n,), generator=g)]
    mask = (torch.rand(n, generator=g) < 0.6).to(torch.uint8)
    mask[0] = mask[n - 1] = 1
    dt = DTYPES[dtype_name]
    acc = acc_dtype(dtype_name)
    return SimpleNamespace(
        n=n, d=d, name=dtype_name, A64=A64, w64=w64, z64=z64, y64=y64, m64=m64,
        A=A64.to(torch.float32).to(dt).contiguous(), w=w64.to(acc),
        m=m64.to(acc), y=y64.to(torch.float32), sw=sw, mask=mask, acc=acc)


def poison_rows(p, rows):
    """Copy of the features with ``rows`` overwritten by NaN / +inf / -inf
    (f64 view and kernel dtype; fp8 e4m3fn has no inf, it gets NaN)."""
    A64 = p.A64.clone()
    pat = torch.tensor([float("nan"), float("inf"), float("-inf")],
                       dtype=torch.float64)
    for r in rows:
        A64[r] = pat[torch.arange(p.d) % 3]
    if p.name == "fp8":
        A = p.A.clone().view(torch.uint8)
        A[list(rows)] = 0x7F  # e4m3fn NaN
        A = A.view(torch.float8_e4m3fn)
    else:
        A = A64.to(DTYPES[p.name]).contiguous()
    return A64, A


# --------------------------------------------------------------------------
# CSR problems
# --------------------------------------------------------------------------

#: row lengths around the 16-byte body of k_csr_margins (it needs about 260
#: stored entries), around one wave (64) and the 4-entry groups
CSR_LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 259, 260, 261, 263, 264,
               520, 1027)
CSR_VECTOR_MIN = 256  # shortest row that can take the 16-byte body


def csr_takes_vector_body(k_lo: int, k_hi: int) -> bool:
    """The 16-byte body's entry condition (64 lanes x 4 entries)."""
    return ((k_lo + 3) & ~3) + 4 * 64 <= (k_hi & ~3)


def _finish_csr(rowptr, col, val64, w64, d, g):
    n = rowptr.numel() - 1
    counts = torch.diff(rowptr)
    rows = torch.repeat_interleave(torch.arange(n), counts)
    terms = val64 * w64[col]
    z64 = torch.zeros(n, dtype=torch.float64).index_add_(0, rows, terms)
    absz = torch.zeros(n, dtype=torch.float64).index_add_(0, rows, terms.abs())
    _check_range(absz)
    y64 = _labels_for(z64, g, flip_interior=False)
    m64 = _nonzero_ints((n,), g)
    sw = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n,), generator=g)]
    mask = (torch.rand(n, generator=g) < 0.6).to(torch.uint8)
    mask[0] = mask[n - 1] = 1
    A64 = torch.zeros((n, d), dtype=torch.float64).index_put_(
        (rows, col), val64, accumulate=True)
    return SimpleNamespace(
        n=n, d=d, rowptr=rowptr.to(torch.int32), col=col.to(torch.int32),
        val=val64.to(torch.float32), val64=val64, rows=rows, w64=w64,
        w=w64.to(torch.float32), z64=z64, y64=y64, y=y64.to(torch.float32),
        m64=m64, m=m64.to(torch.float32), sw=sw, mask=mask, A64=A64)


def csr_eval64(p, loss_type, mask=None, sw=None):
    m, l = mult_loss64(p.z64, p.y64, loss_type)
    m, l, cnt = apply_mask_weight64(m, l, p.n, mask, sw)
    return csr_grad64(p, m), torch.stack([l.sum(), cnt]), m


def csr_grad64(p, m64):
    terms = p.val64 * m64[p.rows]
    col = p.col.long()
    bound = torch.zeros(p.d, dtype=torch.float64).index_add_(0, col, terms.abs())
    _check_range(torch.zeros(1), bound)
    return torch.zeros(p.d, dtype=torch.float64).index_add_(0, col, terms)


@functools.lru_cache(maxsize=None)
def csr_tail_problem(seed: int = 0):
    """One shard with every length of CSR_LENGTHS four times, each time at
    another row start modulo 4 (a 1-entry row between the repeats shifts the
    start by 3571 = 3 mod 4), empty rows at the start, in the middle and at
    the end, one column without any entry, and duplicate column indices
    within rows (the long rows are longer than d). Every stored value and
    every w entry is non-zero; the first / last entry of a row sit in column
    0 / d-1; the last 4-entry group of every long row has a non-zero sum."""
    g = _gen(4242 + seed)
    d, empty_col = 301, 7
    lengths = [0, 0]
    for rep in range(4):
        lengths += list(CSR_LENGTHS) + [1]
    lengths += [0, 0]
    counts = torch.tensor(lengths)
    rowptr = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(counts, 0)
    nnz = int(rowptr[-1])
    w64 = _nonzero_ints((d,), g)
    col = torch.randint(0, d - 1, (nnz,), generator=g)
    col = col + (col >= empty_col).long()  # skips empty_col, reaches d-1
    val64 = _nonzero_ints((nnz,), g)
    for r, ln in enumerate(lengths):
        lo, hi = int(rowptr[r]), int(rowptr[r + 1])
        if ln == 0:
            continue
        seg = col[lo:hi].sort().values
        seg[-1] = d - 1
        if ln > 1:
            seg[0] = 0
        col[lo:hi] = seg
        if ln >= 8 and float((val64[hi - 4:hi] * w64[col[hi - 4:hi]]).sum()) == 0:
            val64[hi - 1] = -val64[hi - 1]
    p = _finish_csr(rowptr, col, val64, w64, d, g)
    p.empty_col = empty_col
    p.lengths = lengths
    return p


#: entries per column of the heavy shard. With CSC_HEAVY_T = CSC_TASK_S = 2048
#: the columns above 2048 entries are split into tasks of 2048, 2048 and a
#: rest (1, 3, 2, 904 entries), whose starts fall on every residue modulo 4.
HEAVY_COL_COUNTS = (3, 2047, 2048, 2049, 1, 5000, 1, 2049, 0, 2051, 2, 2050, 5)
HEAVY_S = 2048


@functools.lru_cache(maxsize=None)
def csr_heavy_problem(seed: int = 0):
    g = _gen(777 + seed)
    n, d = 5000, len(HEAVY_COL_COUNTS)
    rr, cc = [], []
    for c, k in enumerate(HEAVY_COL_COUNTS):
        rr.append(torch.randperm(n, generator=g)[:k].sort().values)
        cc.append(torch.full((k,), c))
    rr, cc = torch.cat(rr), torch.cat(cc)
    order = torch.argsort(rr * d + cc)
    rr, cc = rr[order], cc[order]
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(rr, minlength=n), 0)
    val64 = _nonzero_ints((rr.numel(),), g)
    w64 = _nonzero_ints((d,), g)
    p = _finish_csr(rowptr, cc, val64, w64, d, g)
    p.col_counts = torch.bincount(cc, minlength=d)
    return p


# --------------------------------------------------------------------------
# deliberately sloppy oracles (what a kernel that loses a tail would return)
# --------------------------------------------------------------------------

def sloppy_drop_last_row(p):
    """(margins, grad) of a kernel that never visits the last row."""
    z = p.z64.clone()
    z[-1] = 0.0
    m = p.m64.clone()
    m[-1] = 0.0
    return z, p.A64.T @ m


def sloppy_drop_last_column(p):
    z = p.A64[:, :-1] @ p.w64[:-1]
    gr = p.A64.T @ p.m64
    gr[-1] = 0.0
    return z, gr


def sloppy_drop_slab(p, slab_w: int, slab: int):
    """Margins without the columns of one slab; gradient with that slab's
    entries left at zero."""
    keep = torch.ones(p.d, dtype=torch.bool)
    keep[slab * slab_w:(slab + 1) * slab_w] = False
    z = p.A64[:, keep] @ p.w64[keep]
    gr = (p.A64.T @ p.m64) * keep.double()
    return z, gr


def sloppy_csr_drop_last_group(p, row: int):
    """CSR margins with the last 4-entry group of ``row`` left out."""
    hi = int(p.rowptr[row + 1])
    z = p.z64.clone()
    z[row] -= (p.val64[hi - 4:hi] * p.w64[p.col[hi - 4:hi].long()]).sum()
    return z


def sloppy_csr_double_count(p, row: int):
    """CSR margins with the last entry of ``row`` counted twice."""
    hi = int(p.rowptr[row + 1])
    z = p.z64.clone()
    z[row] += p.val64[hi - 1] * p.w64[int(p.col[hi - 1])]
    return z


# --------------------------------------------------------------------------
# n-space kernels: margin set, extended-precision oracle, error units
# --------------------------------------------------------------------------

def nspace_margins(dtype: torch.dtype):
    """(z [2k], y [2k]): the fixed margin array crossed with y in {0, 1}."""
    f = np.float32 if dtype == torch.float32 else np.float64
    one = f(1.0)
    base = [0.0, 2.0 ** -20, 1.0, float(np.nextafter(one, f(2))),
            float(np.nextafter(one, f(0))), 10.0, 20.0, 87.0, 89.0, 104.0,
            1e4, 3e38, float("inf")]
    vals = [v for b in base for v in (b, -b)]
    z = torch.tensor(vals, dtype=torch.float64).to(dtype)
    k = z.numel()
    return torch.cat([z, z]), torch.cat([torch.zeros(k), torch.ones(k)])


def nspace_oracle(z: torch.Tensor, y: torch.Tensor, loss_type: int):
    """(m, l) as numpy longdouble arrays from the stored margins: the four
    binary losses in x87 extended precision (64-bit mantissa), with the
    overflow-stable softplus."""
    L = np.longdouble
    zz = z.double().numpy().astype(L)
    yy = y.double().numpy().astype(L)
    with np.errstate(over="ignore", invalid="ignore"):
        if loss_type == 0:
            m = L(1) / (L(1) + np.exp(-zz)) - yy
            t = np.where(yy > 0, -zz, zz)
            l = np.where(t > 0, t + np.log1p(np.exp(-np.abs(t))),
                         np.log1p(np.exp(-np.abs(t))))
        elif loss_type == 1:
            m = L(2) * (zz - yy)
            l = (zz - yy) ** 2
        else:
            s = L(2) * yy - L(1)
            sz = s * zz
            if loss_type == 2:
                m = np.where(sz < 1, -s, L(0))
                l = np.where(sz < 1, L(1) - sz, L(0))
            else:
                m = np.where(sz >= 1, L(0), np.where(sz > 0, -s * (1 - sz), -s))
                l = np.where(sz >= 1, L(0),
                             np.where(sz > 0, L(0.5) * (1 - sz) ** 2,
                                      L(0.5) - sz))
    return m, l


def unit_errors(got: torch.Tensor, oracle: np.ndarray, unit: float):
    """|got - oracle| in units of ``unit * max(1, |oracle|)`` per element.
    Where the oracle rounds to +-inf in ``got``'s dtype, or is not finite,
    ``got`` must be that very value: the error is 0 if so, inf if not."""
    g = got.detach().cpu()
    fin = np.finfo(np.float32 if g.dtype == torch.float32 else np.float64)
    L = np.longdouble
    gg = g.double().numpy().astype(L)
    rounded = oracle.copy()
    over = np.abs(oracle) > L(fin.max)
    rounded[over] = np.copysign(L(np.inf), oracle[over])
    out = np.zeros(gg.shape, dtype=np.float64)
    special = ~np.isfinite(rounded)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(gg - oracle) / (L(unit) * np.maximum(L(1), np.abs(oracle)))
    out[~special] = err[~special].astype(np.float64)
    out[special] = np.where(gg[special] == rounded[special], 0.0, np.inf)
    return out
