"""GPU tests of the merged-group kernels' two accumulator forms (DevCSR::mg_acc).

The lanes of ts_stage0 / ts_inner / spmv_merged keep one fp64 accumulator per (segment, row) of
their group either in registers, every product offered to every accumulator through a select
(SSS_HIP_MERGE_ACC=0, sss_spmv_dev.hpp merged_sums), or in LDS, every product added to its own
accumulator only (SSS_HIP_MERGE_ACC=1, merged_sums_lds).  The second form drops only additions of
+0.0 to accumulators that are never -0.0, so every result must be the same bit for bit:
  * one smoother call per level (C/F-Jacobi and its two-stage form), random b and x0;
  * whole cycles (hybrid smoother, direct coarse solve): iterate and residual norm;
  * subnormal products and partial sums, and signed zeros (this decides whether the LDS unit's own
    fp64 add may be used).
Every matrix is forced onto merged groups, for G = 4, 8 rows per group and W = 1, 2, 4 waves per
group.  The hierarchies are chosen (and asserted, host-side) to contain a level whose row count
is no multiple of G, a group of fewer than 64 entries and a group whose per-wave share is no
multiple of the 512 entries a wave takes per iteration.
"""
from __future__ import annotations

import numpy as np
import pytest

import amg_amd as A
from amg_amd._native import csr_arrays
from conftest import build_hierarchy

pytestmark = pytest.mark.gpu

GS = (4, 8)
WS = (1, 2, 4)


@pytest.fixture(scope="module")
def p26_h(quiet):
    return build_hierarchy(A.generate(7, 26), quiet)


@pytest.fixture(scope="module")
def a27_h(quiet):
    return build_hierarchy(A.generate(27, 13), quiet)


@pytest.fixture(params=[(g, w) for g in GS for w in WS], ids=lambda p: f"G{p[0]}W{p[1]}")
def merged(request, monkeypatch):
    """every matrix of the hierarchy on merged row groups of G rows, W waves per group"""
    g, w = request.param
    monkeypatch.setenv("SSS_HIP_WAVE_MIN", "1")
    monkeypatch.setenv("SSS_HIP_FREE_MIN", "1")
    monkeypatch.setenv("SSS_HIP_MERGE_MIN_ROWS", "1")
    monkeypatch.setenv("SSS_HIP_MERGE_G", str(g))
    monkeypatch.setenv("SSS_HIP_MERGE_W", str(w))
    return g, w


def _group_lengths(H, l, g):
    rp, _, _ = csr_arrays(H.level(l).A)
    n = len(rp) - 1
    return n, rp[np.minimum(np.arange(g, n + g, g), n)] - rp[np.arange(0, n, g)]


def _assert_edge_shapes(H, g, w):
    """the tested levels (all but the coarsest) hold the shapes the kernels can go wrong at"""
    levels = [_group_lengths(H, l, g) for l in range(H.num_levels - 1)]
    assert any(n % g for n, _ in levels), "no level with a partial last group"
    assert any((lens < 64).any() for _, lens in levels), "no group shorter than a wave"
    assert any((((lens + w - 1) // w) % 512 != 0).any() for _, lens in levels), "every share a multiple of 512"


def _both_forms(monkeypatch, run):
    out = []
    for acc in ("0", "1"):
        monkeypatch.setenv("SSS_HIP_MERGE_ACC", acc)
        out.append(run())
    return out


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64),
                          np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def _smooth_levels(H, inner, levels, data):
    """x after one pre and one post smoother call on each of `levels`; data(n) -> (b, x0)"""
    D = A.DeviceHierarchy(H, smoother="jacobi", coarse="direct", relabel=1, inner=inner, inner_from=0, sum_order=1)
    out = []
    try:
        assert any(D.level_info(l).a_format & 8 for l in range(H.num_levels - 1))   # merged copies exist
        for l in levels:
            n = H.level(l).A.num_rows
            for post in (False, True):
                b, x0 = data(n)
                D.upload(l, "b", b)
                D.upload(l, "x", x0)
                D.smooth(l, post)
                out.append(D.download(l, "x"))
    finally:
        D.close()
    return out


@pytest.mark.parametrize("hname", ["p26_h", "a27_h"])
@pytest.mark.parametrize("inner", [1, 0])
def test_smoothers_bitwise_equal(request, monkeypatch, hname, inner, merged):
    H = request.getfixturevalue(hname)
    _assert_edge_shapes(H, *merged)

    def run():
        rng = np.random.default_rng(11)
        return _smooth_levels(H, inner, range(H.num_levels - 1),
                              lambda n: (rng.standard_normal(n), rng.standard_normal(n)))

    reg, lds = _both_forms(monkeypatch, run)
    assert len(reg) == len(lds) == 2 * (H.num_levels - 1)
    for k, (xr, xl) in enumerate(zip(reg, lds)):
        assert np.isfinite(xr).all() and np.any(xr != 0.0)
        assert _same_bits(xr, xl), (k // 2, "post" if k % 2 else "pre")


@pytest.mark.parametrize("hname", ["p26_h", "a27_h"])
def test_cycles_bitwise_equal(request, monkeypatch, hname, merged):
    H = request.getfixturevalue(hname)
    _assert_edge_shapes(H, *merged)
    n = H.level(0).A.num_rows

    def run():
        D = A.DeviceHierarchy(H, smoother="hybrid", coarse="direct", sum_order=1)
        try:
            assert any(D.level_info(l).a_format & 8 for l in range(H.num_levels - 1))
            D.upload(0, "b", np.ones(n))
            D.upload(0, "x", np.ones(n))
            for _ in range(3):
                D.cycle()
            return D.download(0, "x"), D.residual_norm()
        finally:
            D.close()

    (x_reg, r_reg), (x_lds, r_lds) = _both_forms(monkeypatch, run)
    assert np.isfinite(r_reg) and r_reg > 0.0
    assert _same_bits(x_reg, x_lds)
    assert _same_bits([r_reg], [r_lds])


@pytest.mark.parametrize("hname", ["p26_h", "a27_h"])
@pytest.mark.parametrize("inner", [1, 0])
def test_subnormal_and_signed_zero_bitwise_equal(request, monkeypatch, hname, inner, merged):
    """Level 1 (a Galerkin level: many distinct values).  b and x0 scaled by 2^-1040: every product
    and partial sum is subnormal; then x0 = 0 with -0.0 entries in b: every product is a signed zero."""
    H = request.getfixturevalue(hname)
    scale = 2.0 ** -1040

    def tiny():
        rng = np.random.default_rng(12)
        return _smooth_levels(H, inner, [1], lambda n: (scale * rng.standard_normal(n), scale * rng.standard_normal(n)))

    def zeros():
        rng = np.random.default_rng(13)

        def data(n):
            b = rng.standard_normal(n)
            b[rng.random(n) < 0.5] = -0.0
            return b, np.zeros(n)
        return _smooth_levels(H, inner, [1], data)

    reg, lds = _both_forms(monkeypatch, tiny)
    for xr, xl in zip(reg, lds):
        assert np.any(xr != 0.0) and np.abs(xr).max() < 2.0 ** -1022   # subnormal results, not flushed
        assert _same_bits(xr, xl)
    reg, lds = _both_forms(monkeypatch, zeros)
    for xr, xl in zip(reg, lds):
        assert _same_bits(xr, xl)
