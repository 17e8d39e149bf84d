"""CPU tests of coarse_direct_cases.py: the reference the GPU tests of the explicit coarse inverse
measure against, and the reasons its matrices were chosen."""
from __future__ import annotations

import numpy as np
import pytest

import coarse_direct_cases as cd


@pytest.mark.parametrize("n", [8, 33])
def test_ld_solve_against_mpmath(n):
    """ld_solve against a 50-digit solve.  Bound: LU with partial pivoting is backward stable up to
    the growth factor, |dx| / |x| <= c n rho cond(A) eps; c n rho is taken as 8 n (rho is of order
    one for a Gaussian matrix), eps is np.longdouble's."""
    import mpmath as mp

    A = cd.dense(cd.gauss(n, 100 + n))
    b = np.random.default_rng(n).standard_normal(n)
    x = cd.ld_solve(A, b)
    assert x.dtype == np.longdouble
    with mp.workdps(50):
        xm = mp.lu_solve(mp.matrix(A.tolist()), mp.matrix(b.tolist()))
        x_ref = np.array([np.longdouble(mp.nstr(v, 30)) for v in xm])
    err = np.linalg.norm((x - x_ref).astype(np.float64)) / np.linalg.norm(x_ref.astype(np.float64))
    bound = 8 * n * np.linalg.cond(A) * np.finfo(np.longdouble).eps
    print(f"n={n}: |x_ld - x_mp| / |x_mp| = {err:.2e}, bound {bound:.2e}")
    assert err <= bound


@pytest.mark.parametrize("n", [1, 2, 3, 65, 257])
def test_shift_closed_form(n):
    A = cd.dense(cd.shift(n))
    b = cd.shift_rhs(n)
    x = cd.shift_solution(n, b)
    assert np.array_equal(cd.ld_solve(A, b), x.astype(np.longdouble))
    assert np.array_equal(A @ x, b)


@pytest.mark.parametrize("n", [2, 3, 65, 257])
def test_shift_pivots_every_column_in_one_cycle(n):
    """Every column but the last swaps rows k and k + 1: overlapping transpositions."""
    _, swaps = cd.gj_inverse(cd.dense(cd.shift(n)))
    assert np.array_equal(swaps, np.minimum(np.arange(n) + 1, n - 1))


@pytest.mark.parametrize("n", [3, 65, 257])
def test_restated_kernel_reproduces_shift_only_with_reverse_unscramble(n):
    """Why `shift` is the exact case: the kernels' algorithm gives the closed form to the bit, and
    the same algorithm with the column swaps undone in forward order does not."""
    A = cd.dense(cd.shift(n))
    b = cd.shift_rhs(n)
    x = cd.shift_solution(n, b)
    inv, _ = cd.gj_inverse(A)
    assert np.array_equal(inv @ b, x)
    assert np.array_equal(inv @ A, np.eye(n))
    fwd, _ = cd.gj_inverse(A, unscramble="forward")
    assert not np.array_equal(fwd @ b, x)


def test_disjoint_transpositions_would_not_tell_the_orders_apart():
    """A permutation made of disjoint row pairs: forward and reverse unscrambling agree, which is
    why `shift` uses one long cycle."""
    n = 64
    A = np.zeros((n, n))
    i = np.arange(n)
    A[i, i ^ 1] = cd.shift_scale(n)
    rev, swaps = cd.gj_inverse(A)
    fwd, _ = cd.gj_inverse(A, unscramble="forward")
    assert np.count_nonzero(swaps != i) == n // 2
    assert np.array_equal(rev, fwd)


@pytest.mark.parametrize("n", [65, 257])
def test_random_cases_pivot_and_fill(n):
    for csr in (cd.sparse_shift(n, n), cd.gauss(n, n)):
        A = cd.dense(csr)
        inv, swaps = cd.gj_inverse(A)
        assert np.count_nonzero(swaps != np.arange(n)) > n // 2
        assert np.count_nonzero(inv) > 0.9 * n * n
        b = np.random.default_rng(1).standard_normal(n)
        x = cd.ld_solve(A, b).astype(np.float64)
        assert np.linalg.norm(inv @ b - x) <= 1e-9 * np.linalg.norm(x)
    assert np.count_nonzero(np.diag(cd.dense(cd.sparse_shift(n, n)))) < n // 4


def test_with_duplicates_is_the_same_matrix():
    csr = cd.sparse_shift(65, 65)
    dup = cd.with_duplicates(csr)
    assert len(dup[2]) > len(csr[2])
    assert dup[0][-1] == len(dup[1]) == len(dup[2])
    assert np.any(dup[1][1:] == dup[1][:-1])   # an entry stored twice in a row
    assert np.array_equal(cd.dense(dup), cd.dense(csr))
