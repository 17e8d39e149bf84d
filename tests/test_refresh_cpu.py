"""Refresh of a set-up hierarchy for new operator values on the same pattern (SSS_amg_refresh, frozen
P and R), host side: the refreshed chain against SSS_blas_mat_rap, against a fresh
setup under a power-of-two scaling, the convergence of the refreshed hierarchy against a fresh one,
the host values-only product (sss_rap_values_host) bit for bit and at any thread count, the error
returns, and the hierarchy file."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import amg_amd as A
import refresh_cases as RC
from conftest import oracle_solve, quiet_ctx

ROOT = Path(__file__).resolve().parent.parent
ERROR_INPUT_PAR, ERROR_DATA_STRUCTURE = -12, -21


@pytest.mark.parametrize("name", RC.CPU_MATRICES)
def test_refresh_to_a_scaled_operator_is_the_fresh_setup(name):
    """Every setup decision is invariant under a power-of-two scaling and every product scales
    exactly, so the refreshed hierarchy is the fresh one byte for byte."""
    M = RC.matrix(name)
    M4 = RC.scaled(M, 4.0)
    H = RC.hierarchy(M)
    H.refresh(M4.mat)
    F = RC.hierarchy(M4.mat)
    assert H.num_levels == F.num_levels
    assert RC.digest(H) == RC.digest(F)
    H.close()
    F.close()


@pytest.mark.parametrize("name", RC.CPU_MATRICES)
@pytest.mark.parametrize("amp,shift", RC.DRIFTS)
def test_refreshed_chain_and_convergence(name, amp, shift, capfd):
    M = RC.matrix(name)
    N = RC.drifted(M, amp, shift)
    H = RC.hierarchy(M)
    frozen = [(A.csr_arrays(H.level(l).P), A.csr_arrays(H.level(l).R), RC.cfmark(H, l)) for l in range(H.num_levels - 1)]
    patterns = [A.csr_arrays(H.level(l).A)[:2] for l in range(H.num_levels)]
    capfd.readouterr()
    H.refresh(N.mat)
    assert capfd.readouterr().out == ""   # nothing on stdout
    assert np.array_equal(A.csr_arrays(H.level(0).A)[2].view(np.uint64), N.v.view(np.uint64))
    lib = A.lib()
    for l in range(H.num_levels - 1):
        L = H.level(l)
        for got, want in zip(A.csr_arrays(L.P) + A.csr_arrays(L.R), frozen[l][0] + frozen[l][1]):
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (name, l)
        assert np.array_equal(RC.cfmark(H, l), frozen[l][2])
        Ch = lib.SSS_blas_mat_rap(C.byref(L.R), C.byref(L.A), C.byref(L.P))
        try:
            assert RC.same_bits(H.level(l + 1).A, Ch), (name, amp, shift, l)
        finally:
            lib.SSS_mat_destroy(C.byref(Ch))
    for l in range(H.num_levels):   # no pattern moved
        for got, want in zip(A.csr_arrays(H.level(l).A)[:2], patterns[l]):
            assert np.array_equal(got, want)
    F = RC.hierarchy(N.mat)
    n = M.num_rows
    b = np.random.default_rng(1).standard_normal(n)
    rtn_f, rel_f, _ = oracle_solve(F, b, np.zeros(n))
    rtn_r, rel_r, _ = oracle_solve(H, b, np.zeros(n))
    print(f"{name} drift ({amp}, {shift}): fresh {rtn_f.nits} iterations, refreshed {rtn_r.nits}")
    assert rel_f[-1] < F.pars.tol
    assert rel_r[-1] < H.pars.tol
    assert rtn_r.nits <= rtn_f.nits + 3
    H.close()
    F.close()


@pytest.mark.parametrize("name", RC.CPU_MATRICES)
def test_host_twin_is_the_host_product_on_every_level(name):
    H = RC.hierarchy(RC.matrix(name))
    for l in range(H.num_levels - 1):
        L = H.level(l)
        Ch = RC.host_rap(L.R, L.A, L.P)
        try:
            Cv = RC.pattern_copy(Ch)
            A.rap_values(L.R, L.A, L.P, Cv.mat)
            assert RC.same_bits(Cv.mat, Ch), (name, l)
        finally:
            A.lib().SSS_mat_destroy(C.byref(Ch))
    H.close()


def test_host_twin_signed_zeros():
    R, Am, P = RC.signed_zero_case()
    Ch = RC.host_rap(R.mat, Am.mat, P.mat)
    try:
        rp, ci, v = A.csr_arrays(Ch)
        assert list(rp) == [0, 3, 5, 7] and list(ci[:3]) == [0, 1, 2]
        assert not np.signbit(v[0]) and v[0] == 0.0      # 0.0 + -0.0
        assert np.signbit(v[1]) and v[1] == 0.0          # -0.0 assigned
        Cv = RC.pattern_copy(Ch)
        A.rap_values(R.mat, Am.mat, P.mat, Cv.mat)
        assert RC.same_bits(Cv.mat, Ch)
    finally:
        A.lib().SSS_mat_destroy(C.byref(Ch))


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import hashlib
import amg_amd as A
import refresh_cases as RC
h = hashlib.sha256()
for name in ["p7_16", "a27_8", "circuit3000"]:
    M = RC.matrix(name)
    H = RC.hierarchy(M)
    N = RC.drifted(M, 0.6, 0.0)   # (owns the arrays: alive across the call)
    H.refresh(N.mat)
    h.update(RC.digest(H).encode())
    for l in range(H.num_levels - 1):
        L = H.level(l)
        Cv = RC.pattern_copy(H.level(l + 1).A)
        A.rap_values(L.R, L.A, L.P, Cv.mat)
        h.update(Cv.v.tobytes())
print("digest", h.hexdigest())
"""


def test_results_do_not_depend_on_the_thread_count():
    out = {}
    for t in ("1", "8"):
        env = dict(os.environ, OMP_NUM_THREADS=t)
        r = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT)], env=env, capture_output=True, text=True, check=True)
        out[t] = [l for l in r.stdout.splitlines() if l.startswith("digest")]
        assert len(out[t]) == 1, r.stdout + r.stderr
    assert out["1"] == out["8"]


def test_missing_column_is_an_error_and_leaves_the_values():
    H = RC.hierarchy(RC.matrix("p7_12"))
    L = H.level(0)
    Cv = RC.pattern_copy(H.level(1).A, fill=7.0)
    row = 5
    k = int(Cv.rp[row]) + 1                      # an off-diagonal entry of row 5 ...
    unused = sorted(set(range(Cv.mat.num_rows)) - set(Cv.ci[Cv.rp[row]:Cv.rp[row + 1]].tolist()))
    Cv.ci[k] = unused[0]                         # ... renamed to a column the product does not reach
    before = Cv.v.copy()
    with pytest.raises(RuntimeError) as e:
        A.rap_values(L.R, L.A, L.P, Cv.mat)
    assert e.value.rc == ERROR_DATA_STRUCTURE
    assert np.array_equal(Cv.v.view(np.uint64), before.view(np.uint64))
    H.close()


def test_refresh_refuses_another_pattern():
    M = RC.matrix("p7_12")
    H = RC.hierarchy(M)
    d0 = RC.digest(H)
    rp, ci, v = A.csr_arrays(M)
    ci2 = ci.copy()
    k = int(rp[3])
    ci2[k], ci2[k + 1] = ci2[k + 1], ci2[k]      # same entries, another col_idx
    other = A.NumpyCSR(rp, ci2, v * 2.0)
    assert A.lib().SSS_amg_refresh(C.byref(H.mg), C.byref(other.mat)) == ERROR_INPUT_PAR
    with pytest.raises(ValueError):
        H.refresh(other.mat)
    assert RC.digest(H) == d0
    rp3 = rp.copy()
    rp3[-1] -= 1                                 # one entry fewer
    fewer = A.NumpyCSR(rp3, ci[:-1], v[:-1] * 2.0)
    assert A.lib().SSS_amg_refresh(C.byref(H.mg), C.byref(fewer.mat)) == ERROR_INPUT_PAR
    assert RC.digest(H) == d0
    bigger = A.generate(7, 13)
    assert A.lib().SSS_amg_refresh(C.byref(H.mg), C.byref(bigger)) == ERROR_INPUT_PAR
    assert RC.digest(H) == d0
    H.close()


@pytest.mark.skipif(A.device_count() > 0, reason="checks the return without a device")
def test_device_product_without_a_device_is_an_error():
    H = RC.hierarchy(RC.matrix("p7_12"))
    L = H.level(0)
    Cv = RC.pattern_copy(H.level(1).A, fill=7.0)
    with pytest.raises(RuntimeError):
        A.rap_values(L.R, L.A, L.P, Cv.mat, device=True)
    assert np.all(Cv.v == 7.0)
    H.close()


def test_one_level_hierarchy_is_just_the_copy():
    M = A.generate(7, 6)
    pars = A.default_pars()
    pars.max_levels = 1
    with quiet_ctx():
        H = A.Hierarchy(M, pars)
    assert H.num_levels == 1
    N = RC.drifted(M, 0.3, 0.0)
    H.refresh(N.mat)
    assert np.array_equal(A.csr_arrays(H.level(0).A)[2].view(np.uint64), N.v.view(np.uint64))
    H.close()


def test_refreshed_hierarchy_round_trips_through_the_file(tmp_path):
    M = RC.matrix("p7_16")
    H = RC.hierarchy(M)
    N = RC.drifted(M, 0.9, 0.1)
    H.refresh(N.mat)
    path = tmp_path / "h.sssamg"
    H.save(path)
    G = A.Hierarchy.load(path)
    assert G.num_levels == H.num_levels
    assert RC.digest(G) == RC.digest(H)
    G.close()
    H.close()


def test_symbols_exported_declared_and_bound():
    header = (ROOT / "include" / "sss_hip.h").read_text()
    for s in ("sss_hip_rap_values", "sss_rap_values_host", "SSS_amg_refresh", "sss_hip_hier_refresh"):
        assert s in A.ABI_SYMBOLS
        assert getattr(A.lib(), s).argtypes
        assert f"int {s}(" in header
    assert callable(A.Hierarchy.refresh) and callable(A.DeviceHierarchy.refresh) and callable(A.rap_values)
