"""Binary data-pass kernels against an exact f64 oracle at their tail shapes.

The data of ``exact_oracle`` makes f32 arithmetic exact, so every comparison
of a data pass here is ``torch.equal`` (``exact_equal``): dense margins
(VALU and MFMA), the dense transpose gradient, the CSR gathers, the CSC
gradients and the whole least-squares / hinge evaluation. The CPU tier
(``test_exact_oracle.py``) shows that the same comparison reports a lost row,
column, slab or CSR group.

The n-space kernels (``k_multiplier``, ``k_multiplier_sum``,
``k_multiplier_affine``) have transcendentals and are compared per element
in units of ``2^-24 * max(1, |oracle|)`` (``2^-53`` for f64 margins) against
an extended-precision oracle. The allowed count is four times the maximum
error of the same formulas in plain torch on the CPU, and at least 4.
Measured on the margin set of ``exact_oracle.nspace_margins``:

    f32 margins: CPU torch maximum 2.000 units, kernels' maximum 2.000 units
    f64 margins: CPU torch maximum 2.000 units, kernels' maximum 2.000 units

so 8 units are allowed for least squares. Both maxima are the least-squares
loss (z - y)^2 at |z| = 1e4, one rounding of z - y squared. Per loss the
allowed count follows that loss's own CPU maximum; the logistic loss, the
one with exp / log1p, measured 0.758 (CPU) and 0.764 (kernels, __expf) units
at f32 and 0.780 / 0.780 at f64, the multipliers 0.514 and 0.758 on both.
"""

import math

import numpy as np
import pytest
import torch

import exact_oracle as xo
from exact_oracle import HINGE, LSQ, exact_equal
from sparkagd_amd import ops
from sparkagd_amd.data import CSRShard
from sparkagd_amd.ops import reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ["bf16", "f32", "f64", "fp8"]
COMBOS = ["plain", "mask", "weights", "mask+weights"]


def _hip():
    from sparkagd_amd.ops import hiplib

    return hiplib


def _g(t):
    return None if t is None else t.to(DEV)


def _combo(p, combo):
    return (p.mask if "mask" in combo else None,
            p.sw if "weights" in combo else None)


def _margins_raw(A, w, n_slabs, algo, nt=1):
    """The margins-only mode of agd_dense_eval with a caller-chosen slab
    count (the library clamps it; the workspace is n_slabs * n)."""
    h = _hip()
    lib = h.load()
    n, d = A.shape
    out = torch.empty(n_slabs * n, dtype=w.dtype, device=A.device)
    rc = lib.agd_dense_eval(
        h._ptr(A), h._DTYPE_CODE[A.dtype], None, None, None, h._ptr(w), n, d,
        None, None, h._ptr(out), None, None, 1, 0, n_slabs, 0, algo, nt, 1,
        h._ptr(h._red_ws(A.device)), h._stream(A))
    h._check(rc)
    return out[:n]


def _effective_slabs(n, d, name, algo=0):
    """(planned, effective slab count, slab width) as agd_dense_eval splits
    the planner's answer."""
    planned = int(_hip().load().agd_margin_slabs(n, d, xo.DTYPE_CODE[name], algo))
    w = xo.W_FULL[name] if d % xo.W_FULL[name] == 0 else 1
    if planned <= 1:
        return planned, 1, d
    align = 64 * w
    slab_w = -(-d // planned)                 # ceil(d / planned)
    slab_w = -(-slab_w // align) * align      # rounded up to 64 lanes x W
    return planned, -(-d // slab_w), slab_w


def _check_margins_and_eval(p, failures, tag, loss_type=None):
    h = _hip()
    A, w, y = _g(p.A), _g(p.w), _g(p.y)
    if not exact_equal(h.dense_margins(A, w), p.z64):
        failures.append((tag, "margins", p.n, p.d))
    loss_type = loss_type or (LSQ if (p.n + p.d) % 2 else HINGE)
    g64, lc64, _ = xo.dense_eval64(p, loss_type)
    g, lc = h.dense_eval(A, y, w, loss_type)
    if not (exact_equal(g, g64) and exact_equal(lc, lc64)):
        failures.append((tag, f"eval loss {loss_type}", p.n, p.d))


# --------------------------------------------------------------------------
# dense margins (VALU row-group kernel)
# --------------------------------------------------------------------------

MARGIN_ROWS_N = [1, 2, 3, 4, 5, 7, 8, 9, 13]


def _margin_d_values(name):
    w = xo.W_FULL[name]
    return sorted({1, w - 1, w, w + 1, 64 * w, 64 * w + w, 3 * 64 * w + 5})


@pytest.mark.parametrize("nt", ["0", "1"])
@pytest.mark.parametrize("name", NAMES)
def test_dense_margins_row_and_column_tails(name, nt, monkeypatch):
    """Full row groups, tail groups and n < R (R = 4, 8 for fp8) against
    aligned d, the W = 1 fallback of unaligned d and the scalar column tail,
    through dense_margins and through mode 0 of dense_eval."""
    monkeypatch.setenv("SPARKAGD_NT_LOADS", nt)
    failures = []
    for n in MARGIN_ROWS_N:
        for d in _margin_d_values(name):
            _check_margins_and_eval(xo.dense_problem(n, d, name), failures, name)
    assert not failures, failures


@pytest.mark.parametrize("nt", ["0", "1"])
@pytest.mark.parametrize("name,n,d,want", [
    ("bf16", 5, 4104, (3, 1032)),   # three slabs, the last 1032 columns
    ("f32", 3, 777, (4, 9)),        # W = 1 path, four slabs, the last 9
    ("f64", 7, 1031, None),
    ("fp8", 9, 8240, None),
])
def test_dense_margins_short_last_slab(name, n, d, want, nt, monkeypatch):
    monkeypatch.setenv("SPARKAGD_NT_LOADS", nt)
    planned, eff, slab_w = _effective_slabs(n, d, name)
    assert planned > 1 and eff > 1, "the planner must slab this shape"
    last = d - (eff - 1) * slab_w
    assert 0 < last < slab_w, "the last slab must be short"
    if want is not None:
        assert (eff, last) == want
    failures = []
    p = xo.dense_problem(n, d, name)
    _check_margins_and_eval(p, failures, name, LSQ)
    _check_margins_and_eval(p, failures, name, HINGE)
    assert not failures, failures


@pytest.mark.parametrize("nt", ["0", "1"])
def test_dense_margins_grid_stride_second_trip(nt, monkeypatch):
    """More row-group tasks than 8192 blocks x 4 waves."""
    monkeypatch.setenv("SPARKAGD_NT_LOADS", nt)
    n, d = 131077, 8
    assert -(-n // 4) > 8192 * 4
    assert _effective_slabs(n, d, "bf16")[1] == 1
    failures = []
    _check_margins_and_eval(xo.dense_problem(n, d, "bf16"), failures, "bf16",
                            HINGE)
    assert not failures, failures


# --------------------------------------------------------------------------
# MFMA margins
# --------------------------------------------------------------------------

MFMA_N = [1, 31, 32, 33, 127, 128, 129, 200]
MFMA_D = [16, 8192, 8208, 16432]  # one LDS chunk, exact, +16, two chunks +48


def test_mfma_margins_row_tails_and_lds_chunks(monkeypatch):
    """w in {-2..2} survives the kernel's bf16 rounding, so the MFMA margins
    are exact too. Through the public path the planner slabs these thin
    shapes below one 8192-column LDS chunk; the single-slab call makes the
    chunk loop take ceil(d / 8192) trips."""
    monkeypatch.setenv("SPARKAGD_MARGINS_ALGO", "2")
    h = _hip()
    failures = []
    for n in MFMA_N:
        for d in MFMA_D:
            p = xo.dense_problem(n, d, "bf16")
            A, w = _g(p.A), _g(p.w)
            if not exact_equal(h.dense_margins(A, w), p.z64):
                failures.append(("planned slabs", n, d))
            if not exact_equal(_margins_raw(A, w, 1, 2), p.z64):
                failures.append(("one slab", n, d))
            g64, lc64, _ = xo.dense_eval64(p, LSQ)
            g, lc = h.dense_eval(A, _g(p.y), w, LSQ)
            if not (exact_equal(g, g64) and exact_equal(lc, lc64)):
                failures.append(("eval", n, d))
    assert not failures, failures


def test_mfma_margins_slabbed(monkeypatch):
    monkeypatch.setenv("SPARKAGD_MARGINS_ALGO", "2")
    n, d = 33, 16432
    planned = int(_hip().load().agd_margin_slabs(n, d, 0, 2))
    assert planned > 1
    p = xo.dense_problem(n, d, "bf16")
    A, w = _g(p.A), _g(p.w)
    assert exact_equal(_hip().dense_margins(A, w), p.z64)
    for s in (2, 3, planned):  # 2: slabs of 8704 columns, across a chunk
        assert exact_equal(_margins_raw(A, w, s, 2), p.z64), s


# --------------------------------------------------------------------------
# dense gradient
# --------------------------------------------------------------------------

def _check_grad(p, failures, tag):
    h = _hip()
    A = _g(p.A)
    if not exact_equal(h.dense_grad_from_mult(A, _g(p.m)),
                       xo.grad64(p.A64, p.m64)):
        failures.append((tag, "mode 3", p.n, p.d))
    for loss_type in (LSQ, HINGE):
        g64, lc64, _ = xo.dense_eval64(p, loss_type)
        g, lc = h.dense_eval(A, _g(p.y), _g(p.w), loss_type)
        if not (exact_equal(g, g64) and exact_equal(lc, lc64)):
            failures.append((tag, f"eval loss {loss_type}", p.n, p.d))
        z = h.dense_margins(A, _g(p.w))
        g, lc = h.dense_eval_from_margins(A, z, _g(p.y), loss_type)
        if not (exact_equal(g, g64) and exact_equal(lc, lc64)):
            failures.append((tag, f"from margins loss {loss_type}", p.n, p.d))


@pytest.mark.parametrize("nt", ["0", "1"])
@pytest.mark.parametrize("name", NAMES)
def test_dense_grad_column_slab_edges_and_few_rows(name, nt, monkeypatch):
    """d around one 256-lane column slab of a block, for the dtype's W and
    for W = 1; n in {1, 2, 3} clamps the row blocks to n."""
    monkeypatch.setenv("SPARKAGD_NT_LOADS", nt)
    lib = _hip().load()
    w = xo.W_FULL[name]
    failures = []
    for d in sorted({256 * w - w, 256 * w, 256 * w + w, 255, 256, 257}):
        for n in (1, 2, 3, 9):
            n_rb = int(lib.agd_dense_rowblocks(n, d, xo.DTYPE_CODE[name]))
            assert n_rb == n, "the row blocks are clamped to n"
            _check_grad(xo.dense_problem(n, d, name), failures, name)
    assert not failures, failures


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n", [4099, 5000])
def test_dense_grad_uneven_row_blocks(name, n):
    lib = _hip().load()
    w = xo.W_FULL[name]
    failures = []
    for d in (3 * w, 3 * w + 1):
        n_rb = int(lib.agd_dense_rowblocks(n, d, xo.DTYPE_CODE[name]))
        assert n_rb > 1 and n % n_rb != 0, "row blocks must be uneven"
        _check_grad(xo.dense_problem(n, d, name), failures, name)
    assert not failures, failures


def test_dense_grad_grid_stride_second_trip():
    """More (row block x column slab) blocks than the 8192-block cap."""
    n, d = 3, 256 * 8192 + 1
    n_rb = int(_hip().load().agd_dense_rowblocks(n, d, 1))
    assert n_rb * -(-d // 256) > 8192  # d is odd: W = 1, 256 columns a block
    failures = []
    _check_grad(xo.dense_problem(n, d, "f32"), failures, "f32")
    assert not failures, failures


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n,rows", [(13, (1, 6, 11)), (4099, (1, 2047, 4097))])
def test_dense_grad_skips_rows_with_zero_multiplier(name, n, rows):
    """KERNELS.md's contract of the raw path: a row whose multiplier is
    exactly 0 is not read. Such rows hold NaN and +-inf; the gradient equals
    the oracle without them, in mode 3 and in a masked full evaluation, whose
    loss_count leaves them out as well."""
    h = _hip()
    w = xo.W_FULL[name]
    rows = list(rows)
    for d in (3 * w, 64 * w + 5):
        p = xo.dense_problem(n, d, name)
        A64, A = xo.poison_rows(p, rows)
        assert not torch.isfinite(A.to(torch.float32)[rows]).any()
        A = _g(A)
        m64 = p.m64.clone()
        m64[rows] = 0.0
        g = h.dense_grad_from_mult(A, _g(m64.to(p.acc)))
        assert exact_equal(g, xo.grad64(p.A64, m64)), (n, d)
        mask = torch.ones(n, dtype=torch.uint8)
        mask[rows] = 0
        for loss_type in (LSQ, HINGE):
            for sw in (None, p.sw):
                g64, lc64, _ = xo.dense_eval64(p, loss_type, mask, sw)
                g, lc = h.dense_eval(A, _g(p.y), _g(p.w), loss_type, _g(mask),
                                     True, _g(sw))
                assert exact_equal(g, g64), (n, d, loss_type)
                assert exact_equal(lc, lc64), (n, d, loss_type)
                want = float(n - len(rows)) if sw is None else \
                    float(p.sw.double()[mask.bool()].sum())
                assert float(lc[1]) == want


# --------------------------------------------------------------------------
# full evaluation, exact
# --------------------------------------------------------------------------

@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("name", NAMES)
def test_dense_eval_exact(name, combo):
    h = _hip()
    w = xo.W_FULL[name]
    for n, d in ((1023, 3 * 64 * w + 5), (259, 64 * w + w)):
        p = xo.dense_problem(n, d, name)
        mask, sw = _combo(p, combo)
        for loss_type in (LSQ, HINGE):
            g64, lc64, _ = xo.dense_eval64(p, loss_type, mask, sw)
            g, lc = h.dense_eval(_g(p.A), _g(p.y), _g(p.w), loss_type,
                                 _g(mask), True, _g(sw))
            assert exact_equal(g, g64), (n, d, loss_type)
            assert exact_equal(lc, lc64), (n, d, loss_type)
            keep = torch.ones(n) if mask is None else mask.float()
            wts = torch.ones(n) if sw is None else sw
            assert float(lc[1]) == float((keep * wts).double().sum())
            _, lc2 = h.dense_eval(_g(p.A), _g(p.y), _g(p.w), loss_type,
                                  _g(mask), False, _g(sw))
            assert torch.equal(lc, lc2)


@pytest.mark.parametrize("combo", COMBOS)
def test_csr_shard_eval_exact(combo):
    p = xo.csr_tail_problem()
    mask, sw = _combo(p, combo)
    shard = CSRShard(_g(p.rowptr), _g(p.col), _g(p.val), _g(p.y), p.d,
                     sample_weight=_g(sw))
    for loss_type in (LSQ, HINGE):
        g64, lc64, _ = xo.csr_eval64(p, loss_type, mask, sw)
        g, lc = shard.eval(_g(p.w), loss_type, _g(mask))
        assert exact_equal(g, g64) and exact_equal(lc, lc64), loss_type
        keep = torch.ones(p.n) if mask is None else mask.float()
        wts = torch.ones(p.n) if sw is None else sw
        assert float(lc[1]) == float((keep * wts).double().sum())


# --------------------------------------------------------------------------
# CSR
# --------------------------------------------------------------------------

@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
def test_csr_tail_shard_exact(idx_dtype):
    """Rows of 0 .. 1027 entries at every start modulo 4: the scalar path,
    the 16-byte body of k_csr_margins with its head and tail, empty rows, an
    empty column, duplicate columns. Margins, the atomic gradient, the CSC
    gather and the heavy-column split are all exact."""
    h = _hip()
    p = xo.csr_tail_problem()
    rp, col, val = _g(p.rowptr.to(idx_dtype)), _g(p.col), _g(p.val)
    shard = CSRShard(_g(p.rowptr), col, val, _g(p.y), p.d)
    assert shard.csc_heavy["task_idx"].numel() > 0
    assert exact_equal(h.csr_margins(rp, col, val, _g(p.w)), p.z64)
    g64 = xo.csr_grad64(p, p.m64)
    m = _g(p.m)
    assert exact_equal(h.csr_grad_from_mult(rp, col, val, m, p.d), g64)
    assert exact_equal(h.csr_grad_from_mult(rp, col, val, m, p.d,
                                            csc=shard.csc), g64)
    assert exact_equal(h.csr_grad_from_mult(rp, col, val, m, p.d, csc=shard.csc,
                                            csc_heavy=shard.csc_heavy), g64)
    assert float(g64[p.empty_col]) == 0.0
    for loss_type in (LSQ, HINGE):
        e64, lc64, _ = xo.csr_eval64(p, loss_type, p.mask, p.sw)
        for csc, heavy in ((None, None), (shard.csc, None),
                           (shard.csc, shard.csc_heavy)):
            g, lc = h.csr_eval(rp, col, val, _g(p.y), _g(p.w), loss_type,
                               _g(p.mask), p.d, csc, True, _g(p.sw), heavy)
            assert exact_equal(g, e64), (loss_type, csc is None, heavy is None)
            assert exact_equal(lc, lc64)


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
def test_csc_heavy_vector_body_exact(idx_dtype, monkeypatch):
    """Columns of 2047, 2048, 2049, 2050, 2051 and 5000 entries with the
    split at 2048: heavy tasks of 2048 and 904 entries run the 16-byte body
    of k_csc_heavy_partial (dead at the default task size of 128), tasks of
    1 to 3 entries its scalar path."""
    monkeypatch.setattr(CSRShard, "CSC_HEAVY_T", xo.HEAVY_S)
    monkeypatch.setattr(CSRShard, "CSC_TASK_S", xo.HEAVY_S)
    h = _hip()
    p = xo.csr_heavy_problem()
    rp, col, val = _g(p.rowptr.to(idx_dtype)), _g(p.col), _g(p.val)
    shard = CSRShard(_g(p.rowptr), col, val, _g(p.y), p.d)
    assert shard.csc_heavy["task_idx"].numel() > 0
    assert int(shard.csc_heavy["S"]) == xo.HEAVY_S
    g64 = xo.csr_grad64(p, p.m64)
    assert exact_equal(h.csr_grad_from_mult(rp, col, val, _g(p.m), p.d,
                                            csc=shard.csc,
                                            csc_heavy=shard.csc_heavy), g64)
    assert exact_equal(h.csr_grad_from_mult(rp, col, val, _g(p.m), p.d), g64)
    assert exact_equal(h.csr_margins(rp, col, val, _g(p.w)), p.z64)
    for loss_type in (LSQ, HINGE):
        for mask, sw in ((None, None), (p.mask, p.sw)):
            e64, lc64, _ = xo.csr_eval64(p, loss_type, mask, sw)
            g, lc = h.csr_eval(rp, col, val, _g(p.y), _g(p.w), loss_type,
                               _g(mask), p.d, shard.csc, True, _g(sw),
                               shard.csc_heavy)
            assert exact_equal(g, e64) and exact_equal(lc, lc64), loss_type
    g, lc = shard.eval(_g(p.w), LSQ)
    e64, lc64, _ = xo.csr_eval64(p, LSQ)
    assert exact_equal(g, e64) and exact_equal(lc, lc64)


# --------------------------------------------------------------------------
# n-space kernels (tolerance in units, see the module docstring)
# --------------------------------------------------------------------------

def _nspace_entry_points(dtype):
    h = _hip()

    def via_dense(z, y, loss_type, mask=None, sw=None):
        feats = torch.empty((z.numel(), 1), dtype=dtype, device=DEV)
        return h.dense_multiplier_loss(feats, z, y, loss_type, mask, sw)

    def via_sum(z, y, loss_type, mask=None, sw=None):
        m, lc3 = h.multiplier_loss_sum(z, y, loss_type, mask, sw)
        return m, lc3[:2]

    def via_affine(z, y, loss_type, mask=None, sw=None):
        assert mask is None
        return h.gram_mult_affine(z, torch.zeros_like(z), 1.0, 0.0, y,
                                  loss_type, sw)

    eps = {"k_multiplier": via_dense, "k_multiplier_sum": via_sum}
    if dtype == torch.float32:
        eps["k_multiplier_affine"] = via_affine
    return eps


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_nspace_kernels_on_the_margin_set(dtype):
    z, y = xo.nspace_margins(dtype)
    n = z.numel()
    unit = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
    zg, yg = _g(z), _g(y)
    s = 2.0 * y - 1.0
    sz = s.double() * z.double()
    finite = z.abs() <= 1e4
    cpu_max = gpu_max = 0.0
    bad = []
    for loss_type in (0, 1, 2, 3):
        m_o, l_o = xo.nspace_oracle(z, y, loss_type)
        m_c, l_c = reference._multiplier_and_loss(z, y.to(dtype), loss_type)
        cpu_err = max(xo.unit_errors(m_c, m_o, unit).max(),
                      xo.unit_errors(l_c, l_o, unit).max())
        assert math.isfinite(cpu_err)
        cpu_max = max(cpu_max, cpu_err)
        allowed = max(4.0, 4.0 * cpu_err)
        for name, fn in _nspace_entry_points(dtype).items():
            m, lc = fn(zg, yg, loss_type)
            # per-element losses: one launch per element, one read-back
            l = torch.stack([fn(zg[i:i + 1], yg[i:i + 1], loss_type)[1][0]
                             for i in range(n)]).cpu()
            m = m.cpu()
            assert not torch.isnan(m).any() and not torch.isnan(l).any(), name
            assert not torch.isnan(lc).any(), name
            assert float(lc[1]) == n
            em = xo.unit_errors(m, m_o, unit)
            el = xo.unit_errors(l.to(dtype) if dtype == torch.float32 else l,
                                l_o, unit)
            gpu_max = max(gpu_max, em.max(), el.max())
            print(f"nspace {dtype} loss {loss_type} {name}: cpu {cpu_err:.3f} "
                  f"mult {em.max():.3f} loss {el.max():.3f} units")
            if em.max() > allowed or el.max() > allowed:
                bad.append((name, loss_type, float(em.max()), float(el.max()),
                            allowed))
            if loss_type in (2, 3):  # the kink: exact zeros at s*z == 1
                at1 = sz == 1.0
                assert at1.sum() == 2
                assert (m[at1] == 0).all() and (l[at1] == 0).all(), name
            if loss_type == 3:  # branch values at s*z == 0
                at0 = sz == 0.0
                assert at0.sum() == 4
                assert torch.equal(m[at0].double(), -s[at0].double()), name
                assert (l[at0] == 0.5).all(), name
            # the f64 loss sum of the finite margins is the sum of the
            # per-element values (n additions, each within 2^-53 relative)
            mf, lcf = fn(zg[finite].contiguous(), yg[finite].contiguous(),
                         loss_type)
            tot = float(l[finite].double().sum())
            assert abs(float(lcf[0]) - tot) <= n * 2.0 ** -52 * abs(tot), name
            assert torch.equal(mf.cpu(), m[finite])
            # masked entries are exact zeros and leave the count; weights
            if name != "k_multiplier_affine":
                mask = (torch.arange(n) % 3 != 0).to(torch.uint8)
                mm, lcm = fn(zg, yg, loss_type, _g(mask))
                mm = mm.cpu()
                assert (mm[mask == 0] == 0).all() and not torch.isnan(mm).any()
                assert torch.equal(mm[mask == 1], m[mask == 1])
                assert float(lcm[1]) == float(mask.sum())
            sw = torch.full((n,), 2.0)
            mw, lcw = fn(zg, yg, loss_type, None, _g(sw))
            assert torch.equal(mw.cpu(), 2.0 * m) and float(lcw[1]) == 2.0 * n
    print(f"nspace {dtype}: CPU torch maximum {cpu_max:.3f} units, kernels' "
          f"maximum {gpu_max:.3f} units")
    assert not bad, bad


def test_multiplier_sum_third_entry_exact():
    """Σ mult of k_multiplier_sum on exact data (least squares, hinge)."""
    h = _hip()
    p = xo.dense_problem(5000, 12, "f32")
    z = _g(p.z64.float())
    for loss_type in (LSQ, HINGE):
        for mask, sw in ((None, None), (p.mask, p.sw)):
            m64, l64 = xo.mult_loss64(p.z64, p.y64, loss_type)
            m64, l64, cnt = xo.apply_mask_weight64(m64, l64, p.n, mask, sw)
            m, lc3 = h.multiplier_loss_sum(z, _g(p.y), loss_type, _g(mask),
                                           _g(sw))
            assert exact_equal(m, m64)
            assert exact_equal(lc3, torch.stack([l64.sum(), cnt, m64.sum()]))


# --------------------------------------------------------------------------
# Gram trial kernels
# --------------------------------------------------------------------------

GRAM_N = [1, 255, 256, 257, 2 ** 21 + 3]  # the last: past the 8192-block cap


def _quarters(n, g, span=8):
    return torch.randint(-4 * span, 4 * span + 1, (n,), generator=g).double() / 4


@pytest.mark.parametrize("n", GRAM_N)
def test_gram_mult_affine_equals_multiplier_on_materialised_margins(n):
    """a*xm + b*zm is exact for a = 0.75, b = 0.25 and multiples of 1/4, so
    k_multiplier_affine equals k_multiplier on the materialised margins bit
    for bit, for every loss, with and without sample weights."""
    h = _hip()
    g = torch.Generator().manual_seed(n)
    xm, zm = _quarters(n, g), _quarters(n, g)
    z64 = 0.75 * xm + 0.25 * zm
    assert torch.equal(z64.float().double(), z64)
    y = (torch.rand(n, generator=g) < 0.5).float()
    sw = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n,), generator=g)]
    xg, zg, yg, zmat = _g(xm.float()), _g(zm.float()), _g(y), _g(z64.float())
    feats = torch.empty((n, 1), dtype=torch.float32, device=DEV)
    for loss_type in (0, 1, 2, 3):
        for w_arg in (None, _g(sw)):
            m_a, lc_a = h.gram_mult_affine(xg, zg, 0.75, 0.25, yg, loss_type,
                                           w_arg)
            m_r, lc_r = h.dense_multiplier_loss(feats, zmat, yg, loss_type,
                                                None, w_arg)
            assert torch.equal(m_a, m_r), (loss_type, w_arg is None)
            assert torch.equal(lc_a, lc_r), (loss_type, w_arg is None)
            if loss_type in (LSQ, HINGE):  # and the exact oracle
                m64, l64 = xo.mult_loss64(z64, y.double(), loss_type)
                m64, l64, cnt = xo.apply_mask_weight64(
                    m64, l64, n, None, None if w_arg is None else sw)
                assert exact_equal(m_a, m64)
                assert exact_equal(lc_a, torch.stack([l64.sum(), cnt]))


@pytest.mark.parametrize("n", GRAM_N)
def test_gram_state_update_exact(n):
    h = _hip()
    g = torch.Generator().manual_seed(100 + n)
    gm_raw, m_y, xm, zm = (_quarters(n, g) for _ in range(4))
    inv_c, theta, pz, pg = 0.5, 0.25, 0.75, -0.5
    g64 = gm_raw * inv_c
    z64 = pz * zm + pg * g64
    x64 = (1.0 - theta) * xm + theta * z64
    for t in (g64, z64, x64):
        assert torch.equal(t.float().double(), t)
    xb_t = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
    md = torch.full_like(xb_t, float("nan"))
    mstore = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    zm_new, xm_new = torch.full_like(mstore, float("nan")), torch.full_like(mstore, float("nan"))
    h.gram_state_update(_g(gm_raw.float()), _g(m_y.float()), _g(xm.float()),
                        _g(zm.float()), inv_c, theta, pz, pg, xb_t, md, mstore,
                        zm_new, xm_new)
    assert xb_t.dtype == md.dtype == torch.float64
    assert exact_equal(xb_t, g64) and exact_equal(md, m_y)
    assert exact_equal(mstore, m_y)
    assert exact_equal(zm_new, z64) and exact_equal(xm_new, x64)
    z2, x2 = h.at_margin_update(_g(zm.float()), _g(xm.float()),
                                _g(g64.float()), pz, pg, theta)
    assert torch.equal(z2, zm_new) and torch.equal(x2, xm_new)


# --------------------------------------------------------------------------
# empty shard
# --------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_empty_shard_on_the_device(name):
    h = _hip()
    acc = xo.acc_dtype(name)
    d = 40
    A = torch.empty((0, d), dtype=xo.DTYPES[name], device=DEV)
    y = torch.empty(0, device=DEV)
    w = torch.ones(d, dtype=acc, device=DEV)
    g, lc = ops.dense_eval(A, y, w, 0)
    assert g.is_cuda and g.dtype == acc and g.shape == (d,)
    assert not g.any() and not lc.any() and lc.shape == (2,)
    z = ops.dense_margins(A, w)
    assert z.is_cuda and z.shape == (0,) and z.dtype == acc
    g, lc = ops.dense_eval_from_margins(A, z, y, 2)
    assert not g.any() and not lc.any()
    g = h.dense_grad_from_mult(A, torch.empty(0, dtype=acc, device=DEV))
    assert g.shape == (d,) and not g.any()
