"""CPU tier of the exact-data kernel tests: proves the method before any
kernel is trusted to it.

* every generated problem really is in the exact range: the repository's
  f32 ``ops.reference`` path on the CPU equals the f64 oracle bit for bit;
* four deliberately sloppy oracles (a lost row, column, column slab, CSR
  4-entry group / a double-counted element) are each reported unequal by
  ``exact_equal``, the comparison the GPU tests use;
* the planner-independent shape properties the GPU tests rely on hold;
* an empty shard is answered without loading or launching anything.
"""

import numpy as np
import pytest
import torch

import exact_oracle as xo
from sparkagd_amd.data import CSRShard
from sparkagd_amd.ops import reference

DENSE_CASES = [  # (n, d, dtype): small, odd, tails of every dtype
    (1, 1, "f32"), (5, 4104, "bf16"), (3, 777, "f32"), (13, 389, "f64"),
    (9, 3 * 64 * 16 + 5, "fp8"), (200, 16432, "bf16"), (4099, 24, "bf16"),
    (5000, 12, "f32"), (7, 2 * 256 + 2, "f64"), (8, 256 * 16 + 16, "fp8"),
]


@pytest.mark.parametrize("n,d,name", DENSE_CASES)
@pytest.mark.parametrize("loss_type", [xo.LSQ, xo.HINGE])
def test_dense_reference_equals_f64_oracle(n, d, name, loss_type):
    p = xo.dense_problem(n, d, name)
    assert xo.exact_equal(reference.dense_margins(p.A, p.w), p.z64)
    assert xo.exact_equal(reference.dense_grad_from_mult(p.A, p.m),
                          xo.grad64(p.A64, p.m64))
    for mask, sw in [(None, None), (p.mask, None), (None, p.sw), (p.mask, p.sw)]:
        g64, lc64, m64 = xo.dense_eval64(p, loss_type, mask, sw)
        g, lc = reference.dense_eval(p.A, p.y, p.w, loss_type, mask, True, sw)
        assert xo.exact_equal(g, g64)
        assert xo.exact_equal(lc, lc64)
        m, _ = reference.dense_multiplier_loss(
            p.A, reference.dense_margins(p.A, p.w), p.y, loss_type, mask, sw)
        assert xo.exact_equal(m, m64)
    # the generator rules: ends non-zero and met by non-zero w / m
    assert (p.A64[0] != 0).all() and (p.A64[-1] != 0).all()
    assert (p.A64[:, 0] != 0).all() and (p.A64[:, -1] != 0).all()
    assert p.w64[0] != 0 and p.w64[-1] != 0 and (p.m64 != 0).all()
    m_ls, _ = xo.mult_loss64(p.z64, p.y64, xo.LSQ)
    assert (m_ls != 0).all()
    m_h, _ = xo.mult_loss64(p.z64, p.y64, xo.HINGE)
    assert (m_h[:8] != 0).all() and (m_h[-8:] != 0).all()


def _csr_problems():
    return [xo.csr_tail_problem(), xo.csr_heavy_problem()]


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("loss_type", [xo.LSQ, xo.HINGE])
def test_csr_reference_equals_f64_oracle(which, loss_type):
    p = _csr_problems()[which]
    assert xo.exact_equal(reference.csr_margins(p.rowptr, p.col, p.val, p.w),
                          p.z64)
    assert xo.exact_equal(
        reference.csr_grad_from_mult(p.rowptr, p.col, p.val, p.m, p.d),
        xo.csr_grad64(p, p.m64))
    # the dense view of the shard agrees with the entry-wise oracle
    assert torch.equal(p.A64 @ p.w64, p.z64)
    for mask, sw in [(None, None), (p.mask, None), (None, p.sw), (p.mask, p.sw)]:
        g64, lc64, _ = xo.csr_eval64(p, loss_type, mask, sw)
        g, lc = reference.csr_eval(p.rowptr, p.col, p.val, p.y, p.w, loss_type,
                                   mask, p.d, True, sw)
        assert xo.exact_equal(g, g64)
        assert xo.exact_equal(lc, lc64)
    m_ls, _ = xo.mult_loss64(p.z64, p.y64, xo.LSQ)
    m_h, _ = xo.mult_loss64(p.z64, p.y64, xo.HINGE)
    assert (m_ls != 0).all() and (m_h != 0).all()


def test_csr_tail_problem_shape_properties():
    p = xo.csr_tail_problem()
    rp = p.rowptr.tolist()
    lens = [rp[i + 1] - rp[i] for i in range(p.n)]
    assert lens[0] == 0 and lens[-1] == 0 and 0 in lens[2:-2]
    starts = {}
    for r, ln in enumerate(lens):
        starts.setdefault(ln, set()).add(rp[r] % 4)
        if ln >= 259 or ln <= 255:  # 256..258 depend on the start
            assert xo.csr_takes_vector_body(rp[r], rp[r + 1]) == (ln >= 259)
    for ln in xo.CSR_LENGTHS:
        if ln >= xo.CSR_VECTOR_MIN:
            assert starts[ln] == {0, 1, 2, 3}, (ln, starts[ln])
    vec = [r for r in range(p.n) if xo.csr_takes_vector_body(rp[r], rp[r + 1])]
    assert {rp[r] % 4 for r in vec} == {0, 1, 2, 3}
    # 256 takes the body only from an aligned start, 255 never
    assert any(lens[r] == 256 for r in vec)
    assert not any(lens[r] <= 255 for r in vec)
    present = set(p.col.tolist())
    assert p.empty_col not in present and {0, p.d - 1} <= present
    dup = False
    for r in range(p.n):
        seg = p.col[rp[r]:rp[r + 1]]
        dup = dup or seg.unique().numel() < seg.numel()
        if lens[r]:
            assert int(seg[-1]) == p.d - 1
    assert dup
    assert (p.val64 != 0).all() and (p.w64 != 0).all()


def test_csr_heavy_problem_task_layout(monkeypatch):
    """With T = S = 2048 the shard has heavy tasks long enough for the
    16-byte body of k_csc_heavy_partial, starting at every residue mod 4."""
    monkeypatch.setattr(CSRShard, "CSC_HEAVY_T", xo.HEAVY_S)
    monkeypatch.setattr(CSRShard, "CSC_TASK_S", xo.HEAVY_S)
    p = xo.csr_heavy_problem()
    assert tuple(p.col_counts.tolist()) == xo.HEAVY_COL_COUNTS
    sh = CSRShard(p.rowptr, p.col, p.val, p.y, p.d)
    h = sh.csc_heavy
    assert h["cols"].tolist() == [3, 5, 7, 9, 11]
    colptr = sh.csc[0].tolist()
    residues, lengths = set(), []
    for t, i in enumerate(h["task_idx"].tolist()):
        c = h["cols"][i].item()
        lo = colptr[c] + (t - h["taskptr"][i].item()) * xo.HEAVY_S
        hi = min(lo + xo.HEAVY_S, colptr[c + 1])
        lengths.append(hi - lo)
        if xo.csr_takes_vector_body(lo, hi):
            residues.add(lo % 4)
    assert residues == {0, 1, 2, 3}
    assert sorted(set(lengths)) == [1, 2, 3, 904, 2048]
    # the default task size can never reach the 16-byte body
    assert not xo.csr_takes_vector_body(0, 128)


# --- the comparison notices a subtly wrong result --------------------------

SLOPPY_CASES = [(5, 4104, "bf16"), (3, 777, "f32"), (200, 16432, "bf16"),
                (4099, 24, "bf16")]


@pytest.mark.parametrize("n,d,name", SLOPPY_CASES)
def test_sloppy_dense_oracles_are_detected(n, d, name):
    p = xo.dense_problem(n, d, name)
    good_z, good_g = p.z64, xo.grad64(p.A64, p.m64)
    as_kernel = lambda t: t.to(p.acc)  # noqa: E731 - what a kernel would return
    assert xo.exact_equal(as_kernel(good_z), good_z)
    assert xo.exact_equal(as_kernel(good_g), good_g)
    slab_w = 64 * xo.W_FULL[name] if d % xo.W_FULL[name] == 0 else 64
    n_slabs = (d + slab_w - 1) // slab_w
    sloppy = [xo.sloppy_drop_last_row(p), xo.sloppy_drop_last_column(p)]
    sloppy += [xo.sloppy_drop_slab(p, slab_w, s) for s in (0, n_slabs - 1)]
    for z, gr in sloppy:
        assert not xo.exact_equal(as_kernel(z), good_z)
        assert not xo.exact_equal(as_kernel(gr), good_g)


def test_sloppy_csr_oracles_are_detected():
    p = xo.csr_tail_problem()
    rp = p.rowptr.tolist()
    for r in range(p.n):
        if rp[r + 1] - rp[r] < 8:
            continue
        for z in (xo.sloppy_csr_drop_last_group(p, r),
                  xo.sloppy_csr_double_count(p, r)):
            assert not xo.exact_equal(z.to(torch.float32), p.z64)
    # a lost row / a lost last entry in the transpose pass
    good = xo.csr_grad64(p, p.m64)
    m = p.m64.clone()
    m[p.n - 3] = 0.0  # the last non-empty row
    assert not xo.exact_equal(xo.csr_grad64(p, m).float(), good)


def test_exact_equal_is_strict():
    o = torch.tensor([1.0, 2.0], dtype=torch.float64)
    assert xo.exact_equal(torch.tensor([1.0, 2.0]), o)
    assert not xo.exact_equal(torch.tensor([1.0, 2.0 + 2.0 ** -22]), o)
    assert not xo.exact_equal(torch.tensor([1.0]), o)
    assert not xo.exact_equal(torch.tensor([1.0, float("nan")]),
                              torch.tensor([1.0, float("nan")]).double())


def test_poisoned_rows_do_not_reach_the_oracle():
    p = xo.dense_problem(13, 389, "f64")
    A64, A = xo.poison_rows(p, [0, 6, 12])
    m = p.m64.clone()
    m[[0, 6, 12]] = 0.0
    g = xo.grad64(A64, m)
    assert torch.isfinite(g).all()
    assert torch.equal(g, xo.grad64(p.A64, m))
    assert not torch.isfinite(A.double()[6]).any()


# --- n-space oracle -------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("loss_type", [0, 1, 2, 3])
def test_nspace_oracle_and_cpu_error(dtype, loss_type):
    """The extended-precision oracle has no NaN on the margin set, and the
    plain torch evaluation of the same formulas stays within a few units."""
    z, y = xo.nspace_margins(dtype)
    assert z.numel() == 52 and not torch.isnan(z).any()
    m_o, l_o = xo.nspace_oracle(z, y, loss_type)
    assert not np.isnan(m_o).any() and not np.isnan(l_o).any()
    m, l = reference._multiplier_and_loss(z, y.to(dtype), loss_type)
    unit = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
    em, el = xo.unit_errors(m, m_o, unit), xo.unit_errors(l, l_o, unit)
    assert np.isfinite(em).all() and em.max() <= 4
    assert np.isfinite(el).all() and el.max() <= 4


# --- empty shard ------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.float64])
def test_empty_shard_returns_zeros_without_a_launch(dtype, monkeypatch):
    from sparkagd_amd.ops import hiplib

    def no_load():
        raise AssertionError("an empty shard must not reach the kernel library")

    monkeypatch.setattr(hiplib, "load", no_load)
    acc = torch.float64 if dtype == torch.float64 else torch.float32
    d = 37
    A = torch.empty((0, d), dtype=dtype)
    y = torch.empty(0)
    w = torch.ones(d, dtype=acc)
    zero_lc = torch.zeros(2, dtype=torch.float64)
    g, lc = hiplib.dense_eval(A, y, w, 0)
    assert g.dtype == acc and torch.equal(g, torch.zeros(d, dtype=acc))
    assert torch.equal(lc, zero_lc)
    g, lc = hiplib.dense_eval(A, y, w, 0, need_grad=False)
    assert g is None and torch.equal(lc, zero_lc)
    z = hiplib.dense_margins(A, w)
    assert z.shape == (0,) and z.dtype == acc
    g, lc = hiplib.dense_eval_from_margins(A, z, y, 1)
    assert torch.equal(g, torch.zeros(d, dtype=acc)) and torch.equal(lc, zero_lc)
    g = hiplib.dense_grad_from_mult(A, torch.empty(0, dtype=acc))
    assert g.dtype == acc and torch.equal(g, torch.zeros(d, dtype=acc))
