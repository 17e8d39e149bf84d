"""CPU tests for the flexible GMRES feature: the convection-diffusion workload generator, and known
answers of the numpy restatement (fgmres_restatement.py) that the GPU tests compare the engine with.
"""
from __future__ import annotations

import numpy as np
import pytest

import amg_amd as A
import oracle
from amg_amd import workloads
from fgmres_restatement import TOL, assert_margin, convdiff_hierarchy, oracle_fgmres, true_relres


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_convdiff_peclet0_is_the_poisson_generator(n):
    rp, ci, v = workloads.convdiff(n, 0.0)
    rp0, ci0, v0 = A.csr_arrays(A.generate(7, n))
    assert rp.dtype == rp0.dtype and ci.dtype == ci0.dtype and v.dtype == v0.dtype
    assert np.array_equal(rp, rp0) and np.array_equal(ci, ci0)
    assert np.array_equal(v.view(np.uint64), v0.view(np.uint64))


@pytest.mark.parametrize("p", [0.5, 2.0])
def test_convdiff_properties(p):
    import scipy.sparse as sp
    n = 6
    M = A.convdiff_csr(n, p)
    assert M.mat.num_rows == n ** 3 and M.mat.num_nnzs == len(M.v) == 7 * n ** 3 - 6 * n * n
    S = sp.csr_matrix((M.v, M.ci, M.rp), shape=(n ** 3, n ** 3))
    assert all(np.all(np.diff(M.ci[a:b]) > 0) for a, b in zip(M.rp[:-1], M.rp[1:]))   # columns ascending
    assert abs(S - S.T).max() == p   # nonsymmetric: a_ij - a_ji = -p across every link
    d = S.diagonal()
    assert np.all(d == 6.0 + 3.0 * p)
    off = np.asarray(abs(S).sum(axis=1)).ravel() - d
    assert np.all(off <= d)   # weakly diagonally dominant, strictly at the boundary
    r = np.arange(n ** 3)
    i, j, k = r % n, (r // n) % n, r // (n * n)
    interior = (i > 0) & (i < n - 1) & (j > 0) & (j < n - 1) & (k > 0) & (k < n - 1)
    rows = np.asarray(S.sum(axis=1)).ravel()
    assert np.all(rows[interior] == 0.0) and np.all(rows[~interior] > 0.0)
    # the rows are i + n(j + nk): the -x neighbour of an interior row is the upwind one
    q = 1 + n * (1 + n)
    assert S[q, q - 1] == -(1.0 + p) and S[q, q + 1] == -1.0
    assert S[q, q - n] == -(1.0 + p) and S[q, q + n * n] == -1.0


@pytest.fixture(scope="module")
def hier(quiet):
    cache = {}

    def get(n, p):
        if (n, p) not in cache:
            cache[(n, p)] = convdiff_hierarchy(n, p, quiet)
        return cache[(n, p)][1]
    return get


# n, peclet, restart -> iterations of the restatement in exact mode (oracle.opts() defaults), b = 1,
# x0 = 0, tol 1e-6
KNOWN = [(11, 2.0, 20, 5), (11, 2.0, 3, 5), (16, 2.0, 20, 5), (11, 0.0, 20, 3)]


@pytest.mark.parametrize("n,p,restart,want", KNOWN)
def test_restatement_known_answers(hier, n, p, restart, want):
    H = hier(n, p)
    its, hist, x = oracle_fgmres(H, oracle.opts(), TOL, restart)
    print(f"convdiff {n}^3 p={p} FGMRES({restart}): {its} iterations, estimates {hist}")
    assert its == want
    assert_margin(hist, TOL, f"convdiff {n}^3 p={p} restart {restart}")
    assert true_relres(H, x) < TOL


def test_restatement_is_plain_gmres_on_a_small_system(hier):
    """With maxit = 2 the restatement stops at 2 with the iterate of those two columns, and its
    estimate equals the true residual of that iterate (right preconditioning)."""
    H = hier(11, 2.0)
    its, hist, x = oracle_fgmres(H, oracle.opts(), TOL, 20, maxit=2)
    assert its == 2
    assert abs(true_relres(H, x) - hist[-1]) <= 1e-10 * hist[-1]
