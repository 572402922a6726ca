"""The one routing table of the multi-column data passes (margins Z = A·W,
gradient G = Aᵀ·M) over a raw dense GPU block: ``dense_multi_route`` against
a table written out by hand. Pure values, no GPU."""

import pytest
import torch

from sparkagd_amd.ops import multiclass as mc

BF16, F32, F64, FP8 = (torch.bfloat16, torch.float32, torch.float64,
                       torch.float8_e4m3fn)
ALGOS = ("auto", "gemm", "valu", "mfma")
G, M, F, V, X = "gemm", "mm", "fp8_mfma", "valu", NotImplementedError

# (dtype, fp8_served) -> {kc: routes under (auto, gemm, valu, mfma)}.
# fp8_served=True on a dtype other than fp8 cannot come from
# multi_fp8_serves; the rows are there because the function is total.
EXPECTED = {
    (BF16, False): {4: (G, G, V, G), 32: (G, G, V, G),
                    36: (G, G, X, G), 132: (G, G, X, G)},
    (BF16, True): {4: (G, G, V, G), 32: (G, G, V, G),
                   36: (G, G, F, G), 132: (G, G, F, G)},
    (F32, False): {4: (V, V, V, V), 32: (V, V, V, V),
                   36: (M, M, M, M), 132: (M, M, M, M)},
    (F32, True): {4: (V, V, V, F), 32: (V, V, V, F),
                  36: (M, M, M, M), 132: (M, M, M, M)},
    (F64, False): {4: (V, V, V, V), 32: (V, V, V, V),
                   36: (X, X, X, X), 132: (X, X, X, X)},
    (F64, True): {4: (V, V, V, F), 32: (V, V, V, F),
                  36: (F, F, F, F), 132: (F, F, F, F)},
    (FP8, False): {4: (V, V, V, V), 32: (V, V, V, V),
                   36: (X, X, X, X), 132: (X, X, X, X)},
    (FP8, True): {4: (V, V, V, F), 32: (V, V, V, F),
                  36: (F, F, F, F), 132: (F, F, F, F)},
}

CELLS = [(dtype, kc, served, algo, routes[i])
         for (dtype, served), by_kc in EXPECTED.items()
         for kc, routes in by_kc.items()
         for i, algo in enumerate(ALGOS)]


def _route_or_error(dtype, kc, served, algo):
    try:
        return mc.dense_multi_route(dtype, kc, served, algo)
    except NotImplementedError:
        return NotImplementedError


def test_table_is_complete():
    assert len(CELLS) == 4 * 4 * 2 * 4
    assert len({c[:4] for c in CELLS}) == len(CELLS)


@pytest.mark.parametrize("dtype,kc,served,algo,want", CELLS)
def test_dense_multi_route(dtype, kc, served, algo, want):
    assert _route_or_error(dtype, kc, served, algo) == want


# What every input took before the table existed, with both variables unset:
# the five ladders agreed there (bf16: hipBLASLt at every width; f32: VALU
# kernels up to 32 padded columns and torch.mm above; fp8: VALU up to 32, the
# MFMA kernels above when they serve the block, else an error; f64: VALU up
# to 32 (where the kernel itself then refuses f64), an error above).
UNSET = [
    (BF16, False, {4: G, 32: G, 36: G, 132: G}),
    (F32, False, {4: V, 32: V, 36: M, 132: M}),
    (F64, False, {4: V, 32: V, 36: X, 132: X}),
    (FP8, False, {4: V, 32: V, 36: X, 132: X}),
    (FP8, True, {4: V, 32: V, 36: F, 132: F}),
]


@pytest.mark.parametrize("dtype,served,by_kc", UNSET)
def test_unset_environment_keeps_the_present_routes(dtype, served, by_kc):
    for kc, want in by_kc.items():
        assert _route_or_error(dtype, kc, served, "auto") == want, kc


def test_not_implemented_names_the_three_ways_out():
    with pytest.raises(NotImplementedError) as e:
        mc.dense_multi_route(FP8, 36, False, "auto")
    for word in ("bf16", "f32", "fp8", "d % 16 == 0"):
        assert word in str(e.value)


@pytest.mark.parametrize("dtype", [BF16, F32, F64, FP8])
@pytest.mark.parametrize("kc", [4, 36])
def test_unknown_algo_raises(dtype, kc):
    with pytest.raises(ValueError) as e:
        mc.dense_multi_route(dtype, kc, dtype == FP8, "foo")
    for name in ALGOS:
        assert name in str(e.value)


@pytest.mark.parametrize("grad,var", [(False, "SPARKAGD_MULTI_MARGINS"),
                                      (True, "SPARKAGD_MULTI_GRAD")])
def test_each_pass_reads_its_own_variable(grad, var, monkeypatch):
    block = torch.zeros((2, 16), dtype=torch.bfloat16)
    monkeypatch.delenv("SPARKAGD_MULTI_MARGINS", raising=False)
    monkeypatch.delenv("SPARKAGD_MULTI_GRAD", raising=False)
    assert mc._dense_route(block, 3, grad) == "gemm"
    monkeypatch.setenv(var, "valu")
    assert mc._dense_route(block, 3, grad) == "valu"
    assert mc._dense_route(block, 3, not grad) == "gemm"
    monkeypatch.setenv(var, "foo")
    with pytest.raises(ValueError):
        mc._dense_route(block, 3, grad)
