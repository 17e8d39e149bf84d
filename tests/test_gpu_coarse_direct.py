"""GPU tests of the explicit coarse inverse (sss_coarse_direct.hip: Gauss-Jordan with partial
pivoting, column unscramble, one GEMV per apply) on matrices where it has to pivot, through
sss_hip_host_coarse_solve(A, b, x, ctol, 1, 0), which builds and applies it for any host CSR.

- Exact: coarse_direct_cases.shift(n), whose solve is exact in powers of two, at the sizes where the
  kernels change trips: dense_gemv (64 lanes per row, 4 rows per workgroup), gj_eliminate (256-wide
  column blocks), gj_pivot (1024 threads; second and third trips of its strided loops).
- Accuracy: matrices that pivot and fill, the real coarsest matrices of three hierarchies, and one
  with duplicate stored entries.  Reference: LU with partial pivoting in np.longdouble (ld_solve).
  Yardstick: LAPACK's explicit inverse in fp64 on the same matrix, np.linalg.inv(A) @ b -- the same
  class of algorithm (partial pivoting, explicit inverse, same growth).  Asserted:
  ||x_gpu - x_ld|| <= 16 ||x_lapack - x_ld|| and ||A x_gpu - b|| <= 16 ||A x_lapack - b||.  The 16 was
  set before any GPU run, from a numpy restatement of the kernels (ratios 0.8 to 3.3, leaving about
  5x for another summation order); a missing or wrong pivot is orders of magnitude beyond it.
  Measured on an MI355X, (error ratio, residual ratio): sparse_shift 65 (1.25, 1.10), 257 (2.36,
  1.43), 1025 (2.30, 0.91); gauss 65 (1.07, 1.11), 257 (0.42, 1.08), 1025 (2.70, 0.70); coarsest
  matrices 7-pt 32^3 (2.07, 2.06), 27-pt 16^3 (1.74, 1.79), 1138_bus (0.53, 0.81); with_duplicates
  of sparse_shift 257 (2.36, 1.43).  Errors 5e-16 to 6e-11.
- Singular and non-finite matrices fail with a non-zero code and leave x alone; a hierarchy whose
  coarsest matrix is singular falls back to the Krylov coarse solve.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import amg_amd as A
import coarse_direct_cases as cd
from conftest import build_hierarchy, vec

pytestmark = pytest.mark.gpu

RATIO = 16.0
ERROR_SOLVER_EXIT = -49


@pytest.fixture(scope="module", autouse=True)
def _host_cache():
    A.lib().sss_hip_host_cache_clear()
    yield
    A.lib().sss_hip_host_cache_clear()


@pytest.fixture(scope="module")
def bus_h(bus_matrix, quiet):
    return build_hierarchy(bus_matrix, quiet)


@pytest.fixture(scope="module")
def p32_h(quiet):
    return build_hierarchy(A.generate(7, 32), quiet)


@pytest.fixture(scope="module")
def a27_h(quiet):
    return build_hierarchy(A.generate(27, 16), quiet)


def _direct_solve(csr, b, x0=None):
    hold = A.NumpyCSR(*csr)
    x = np.zeros(len(b)) if x0 is None else x0.copy()
    rc = A.lib().sss_hip_host_coarse_solve(C.byref(hold.mat), C.byref(vec(b)), C.byref(vec(x)), 1e-7, 1, 0)
    return rc, x


# ---- exact ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1100, 2100])
def test_shift_is_solved_exactly(n):
    b = cd.shift_rhs(n)
    rc, x = _direct_solve(cd.shift(n), b)
    assert rc == 0
    want = cd.shift_solution(n, b)
    bad = np.flatnonzero(x != want)
    assert np.array_equal(x, want), f"{len(bad)} of {n} entries differ, first at {bad[:5]}"


# ---- accuracy -------------------------------------------------------------------------------
def _norm(v):
    return float(np.sqrt(np.sum(np.asarray(v, np.longdouble) ** 2)))


def _assert_accuracy(name, csr, b, x_gpu):
    D = cd.dense(csr)
    x_ld = cd.ld_solve(D, b)
    x_la = np.linalg.inv(D) @ b
    Dl = D.astype(np.longdouble)
    err_gpu, err_la = _norm(x_gpu - x_ld), _norm(x_la - x_ld)
    res_gpu, res_la = _norm(Dl @ x_gpu - b), _norm(Dl @ x_la - b)
    print(f"{name}: n={len(b)} cond {np.linalg.cond(D):.1e}  error gpu {err_gpu:.3e} lapack {err_la:.3e} "
          f"ratio {err_gpu / err_la:.2f}  residual gpu {res_gpu:.3e} lapack {res_la:.3e} ratio {res_gpu / res_la:.2f}")
    assert np.all(np.isfinite(x_gpu))
    assert err_gpu <= RATIO * err_la
    assert res_gpu <= RATIO * res_la


@pytest.mark.parametrize("n", [65, 257, 1025])
@pytest.mark.parametrize("kind", ["sparse_shift", "gauss"])
def test_pivoting_matrices_against_lapack(kind, n):
    csr = getattr(cd, kind)(n, 7 * n)
    b = np.random.default_rng(n).standard_normal(n)
    rc, x = _direct_solve(csr, b)
    assert rc == 0
    _assert_accuracy(f"{kind}({n})", csr, b, x)


@pytest.mark.parametrize("hname", ["p32_h", "a27_h", "bus_h"])
def test_real_coarsest_matrices_against_lapack(request, hname):
    """p32_h with default_rng(1) is the matrix and right-hand side of test_coarse_direct_solves
    (test_gpu_parity.py), which asserts its residual only: here its forward error too."""
    H = request.getfixturevalue(hname)
    csr = A.csr_arrays(H.level(H.num_levels - 1).A)
    n = len(csr[0]) - 1
    b = np.random.default_rng(1).standard_normal(n)
    rc, x = _direct_solve(csr, b)
    assert rc == 0
    _assert_accuracy(hname, csr, b, x)


def test_duplicate_entries_add_up():
    """The dense expansion adds stored duplicates: halves of an entry give the bits of the whole."""
    n = 257
    csr = cd.sparse_shift(n, 7 * n)
    dup = cd.with_duplicates(csr)
    assert len(dup[2]) > len(csr[2])
    b = np.random.default_rng(n).standard_normal(n)
    rc, x = _direct_solve(csr, b)
    rc_d, x_d = _direct_solve(dup, b)
    assert rc == 0 and rc_d == 0
    assert np.array_equal(x_d.view(np.uint64), x.view(np.uint64))
    _assert_accuracy("with_duplicates(sparse_shift(257))", dup, b, x_d)


# ---- singular and non-finite ----------------------------------------------------------------
def _singular_cases():
    ones2 = (np.array([0, 2, 4], np.int32), np.array([0, 1, 0, 1], np.int32), np.ones(4))
    D = cd.dense(cd.sparse_shift(65, 3))
    # the block [[1, 1], [1, 1]] as a diagonal block: the pivot 1 leaves row 1 exactly zero.  (Twin
    # rows that also hold other entries leave a pivot of rounding size, not zero -- the pivot row is
    # scaled by 1 / pivot before it is subtracted -- and a near-singularity threshold is not tested.)
    D[0:2] = 0.0
    D[:, 0:2] = 0.0
    D[0:2, 0:2] = 1.0
    rp, ci, v = cd.sparse_shift(65, 4)
    vz = v.copy()
    vz[rp[40]:rp[41]] = 0.0   # row 40 stored, all zeros
    rpn, cin, vn = cd.gauss(65, 5)
    vn = vn.copy()
    vn[7 * 65 + 11] = np.nan
    # an Inf in column 0 is the first pivot, and 1 / Inf = 0 wipes the pivot row: the finished
    # "inverse" is all finite and wrong (gj_inverse on the CPU shows it), so only the pivot test sees
    # it.  A NaN spreads, a zero pivot leaves Inf, and an Inf in a later column is spread by the rows
    # pivoted before it: the scan of the inverse sees those too.
    vi = cd.gauss(65, 5)[2].copy()
    vi[7 * 65 + 0] = np.inf
    with np.errstate(all="ignore"):
        assert np.all(np.isfinite(cd.gj_inverse(cd.dense((rpn, cin, vi)))[0]))
    return {"ones2": ones2, "ones2_embedded": cd._csr_from_dense(D), "zero_row": (rp, ci, vz), "nan_entry": (rpn, cin, vn),
            "inf_entry": (rpn, cin, vi)}


@pytest.mark.parametrize("case", ["ones2", "ones2_embedded", "zero_row", "nan_entry", "inf_entry"])
def test_singular_or_nonfinite_matrix_is_an_error(case):
    csr = _singular_cases()[case]
    n = len(csr[0]) - 1
    x0 = np.full(n, 7.0)
    rc, x = _direct_solve(csr, np.arange(1.0, n + 1.0), x0)
    assert rc == ERROR_SOLVER_EXIT
    assert np.array_equal(x, x0)
    # the next call, with a regular matrix, is not disturbed
    b = cd.shift_rhs(65)
    rc, x = _direct_solve(cd.shift(65), b)
    assert rc == 0 and np.array_equal(x, cd.shift_solution(65, b))


def test_hierarchy_with_singular_coarsest_falls_back_to_krylov(quiet, monkeypatch):
    """A coarsest matrix with a zero row: coarse="direct" creates the engine all the same, without
    the single-workgroup tail (which ends in the inverse), and its cycles are those of coarse="krylov"
    bit for bit -- never non-finite iterates from an Inf/NaN inverse under return code 0."""
    monkeypatch.setenv("SSS_HIP_TAIL", "1")
    monkeypatch.setenv("SSS_HIP_TAIL_NNZ", "1000000")   # as test_gpu_tail.py: the tail engages on 24^3
    H = build_hierarchy(A.generate(7, 24), quiet)
    n = H.level(0).A.num_rows
    D = A.DeviceHierarchy(H, smoother="hybrid", coarse="direct")
    assert A.lib().sss_hip_tail_from(D.h) > 0   # untouched: the inverse and the tail
    D.close()
    Ac = H.level(H.num_levels - 1).A
    rp, ci, v = A.csr_arrays(Ac, copy=False)
    v[rp[5]:rp[6]] = 0.0
    out = {}
    for coarse in ("direct", "krylov"):
        D = A.DeviceHierarchy(H, smoother="hybrid", coarse=coarse)
        try:
            assert A.lib().sss_hip_tail_from(D.h) == -1
            D.upload(0, "b", np.ones(n))
            D.upload(0, "x", np.zeros(n))
            for _ in range(3):
                D.cycle()
            out[coarse] = D.download(0, "x")
        finally:
            D.close()
    assert np.all(np.isfinite(out["direct"]))
    assert np.array_equal(out["direct"].view(np.uint64), out["krylov"].view(np.uint64))
