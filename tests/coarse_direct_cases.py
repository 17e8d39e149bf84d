"""What the tests of the explicit coarse inverse (sss_coarse_direct.hip) share: matrices on which its
Gauss-Jordan has to pivot, one extended-precision reference, and a numpy restatement of the kernels'
algorithm.

The coarsest matrices of the hierarchies the suite builds (7-pt 32^3 and 24^3, 27-pt 16^3, 1138_bus)
are diagonally dominant enough that the pivot search never leaves row k: no row is swapped, the column
unscramble moves nothing, and with at most 322 rows no loop strided by 1024 takes a second trip.  The
matrices here make every column pivot.

A matrix is the CSR triple (row_ptr int32, col_idx int32, val float64); `dense` expands it the way
coarse_direct_build does (stored duplicates of an entry add up).
"""
from __future__ import annotations

import numpy as np

# the reference has to be well below fp64: x87 extended precision (64-bit significand) or better
assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than float64 on this platform"


def _csr_from_dense(D):
    """Full-pattern CSR of the non-zeros of D, columns ascending."""
    n = D.shape[0]
    rows, cols = np.nonzero(D)
    rp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    return rp, cols.astype(np.int32), np.ascontiguousarray(D[rows, cols], dtype=np.float64)


def dense(csr):
    rp, ci, v = csr
    n = len(rp) - 1
    D = np.zeros((n, n))
    np.add.at(D, (np.repeat(np.arange(n), np.diff(rp)), ci), v)
    return D


def shift_scale(n):
    """s_j of `shift`: the value stored in column j, a power of two between 1/8 and 8."""
    return 2.0 ** ((np.arange(n) % 7) - 3)


def shift(n):
    """Row i has one entry, at column (i - 1) mod n, with value s_j = 2^((j mod 7) - 3) for that column.

    Column k's only entry sits in row k + 1, so every column but the last swaps rows k and k + 1.  The
    transpositions (0 1), (1 2), ... overlap -- together one cycle of length n -- so undoing them in
    forward order instead of reverse order gives another matrix; disjoint transpositions would not
    tell the two apart (test_coarse_direct_cases.py pins both facts).  All arithmetic is on powers of
    two and zeros, so the inverse and the solve are exact with or without FMA: see shift_solution."""
    i = np.arange(n)
    cols = (i - 1) % n
    return np.arange(n + 1, dtype=np.int32), cols.astype(np.int32), shift_scale(n)[cols]


def shift_rhs(n):
    """Small non-zero integers, none repeated next to itself."""
    return ((np.arange(n) * 5) % 9 + 1.0) * np.where(np.arange(n) % 3 == 1, -1.0, 1.0)


def shift_solution(n, b):
    """x_j = b_((j + 1) mod n) / s_j, exact for small-integer b."""
    return b[(np.arange(n) + 1) % n] / shift_scale(n)


def sparse_shift(n, seed):
    """About 8 N(0,1) entries per row at random columns, plus 3 * (the cyclic shift of `shift`): the
    diagonal is mostly zero, so nearly every column pivots, and the elimination fills the matrix."""
    rng = np.random.default_rng(seed)
    D = np.zeros((n, n))
    per_row = min(8, n)
    for i in range(n):
        D[i, rng.choice(n, per_row, replace=False)] = rng.standard_normal(per_row)
    i = np.arange(n)
    D[i, (i - 1) % n] += 3.0
    return _csr_from_dense(D)


def gauss(n, seed):
    """Dense N(0,1), stored as a full CSR."""
    return _csr_from_dense(np.random.default_rng(seed).standard_normal((n, n)))


def with_duplicates(csr, every=3):
    """The same matrix with every `every`-th stored entry split into two stored entries of the same
    column, each half the value: halving and re-adding is exact, so `dense` of the result is bitwise
    `dense` of the input, provided the builder adds duplicates up."""
    rp, ci, v = csr
    split = np.arange(len(v)) % every == 0
    reps = np.where(split, 2, 1)
    ci2 = np.repeat(ci, reps)
    v2 = np.repeat(np.where(split, 0.5 * v, v), reps)
    cnt = np.add.reduceat(reps, rp[:-1]) if len(v) else np.zeros(len(rp) - 1, int)
    rp2 = np.zeros(len(rp), np.int32)
    np.cumsum(cnt, out=rp2[1:])
    return rp2, ci2.astype(np.int32), np.ascontiguousarray(v2)


def ld_solve(A, b):
    """x of A x = b by LU with partial pivoting, every operation in np.longdouble."""
    M = np.array(A, dtype=np.longdouble)
    y = np.array(b, dtype=np.longdouble)
    n = len(y)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
            y[[k, p]] = y[[p, k]]
        f = M[k + 1:, k] / M[k, k]
        M[k + 1:, k + 1:] -= np.outer(f, M[k, k + 1:])
        y[k + 1:] -= f * y[k]
    x = np.zeros(n, np.longdouble)
    for k in range(n - 1, -1, -1):
        x[k] = (y[k] - M[k, k + 1:] @ x[k + 1:]) / M[k, k]
    return x


def gj_inverse(A, unscramble="reverse"):
    """The kernels' algorithm in fp64 numpy: per column, the first row of maximum |a_ik| (i >= k) is
    swapped into row k, the pivot row is scaled (its pivot entry becoming 1 / pivot), every other row
    takes the rank-1 update in place (its entry in column k becoming -a_ik / pivot); at the end the
    column swaps are undone in reverse order.  `unscramble="forward"` is the mistake the `shift`
    matrix is there to catch."""
    M = np.array(A, dtype=np.float64)
    n = M.shape[0]
    swaps = np.arange(n)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        swaps[k] = p
        if p != k:
            M[[k, p]] = M[[p, k]]
        col = M[:, k].copy()
        inv = 1.0 / col[k]
        M[k] *= inv
        M[k, k] = inv
        others = np.arange(n) != k
        M[others] -= np.outer(col[others], M[k])
        M[others, k] = -col[others] * inv
    order = range(n - 1, -1, -1) if unscramble == "reverse" else range(n)
    for k in order:
        p = swaps[k]
        if p != k:
            M[:, [k, p]] = M[:, [p, k]]
    return M, swaps
