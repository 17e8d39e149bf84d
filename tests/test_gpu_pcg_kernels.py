"""GPU: the two fused level-0 kernels of sss_hip_dist_pcg (sss_blas.hip) on host data, against numpy.

pcg_update  x += a p, r_old = r, r -= a q and r.r in one pass: x, r and r_old bitwise numpy's
            x + a * p, r - a * q and r.copy() with a = num / den rounded once (the operation order
            of the unfused axpy kernels).
dot2        r.z and r_old.z in one pass.

The sums are fixed-order tree sums, so they differ from numpy's by at most the any-order summation
bound of both: 2 gamma_n sum |a_i b_i|, gamma_n = n u / (1 - n u), u = 2^-53.

Shapes as test_host_orth_matches_numpy_cgs2 -- below one workgroup, odd tails, across the grid of
1024 chunks -- plus an even n and one where a thread's loop runs more than once (chunks > 512 rows).
"""
from __future__ import annotations

import numpy as np
import pytest

import amg_amd as A
from amg_amd._native import dptr

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SIZES = [1, 2, 63, 1331, 4096, 4097, 1100003]


def _gamma(n):
    return n * U / (1 - n * U)


@pytest.mark.parametrize("n", SIZES)
def test_pcg_update_matches_numpy(n):
    rng = np.random.default_rng(7000 + n)
    p, q, x, r = (rng.standard_normal(n) for _ in range(4))
    num, den = 0.7310585786300049, 3.0
    a = num / den
    outs = []
    for _ in range(2):
        xo, ro, rold, rr = x.copy(), r.copy(), np.full(n, np.nan), np.zeros(1)
        assert A.lib().sss_hip_host_pcg_update(n, num, den, dptr(p), dptr(q), dptr(xo), dptr(ro), dptr(rold), dptr(rr)) == 0
        outs.append((xo, ro, rold, rr[0]))
    (xo, ro, rold, rr), (x2, r2, rold2, rr2) = outs
    r_new = r - a * q
    assert np.array_equal(xo.view(np.uint64), (x + a * p).view(np.uint64))
    assert np.array_equal(ro.view(np.uint64), r_new.view(np.uint64))
    assert np.array_equal(rold.view(np.uint64), r.view(np.uint64))
    bound = 2 * _gamma(n) * np.dot(r_new, r_new)
    print(f"n={n}: |rr - numpy| / bound = {abs(rr - np.dot(r_new, r_new)) / bound:.3f}")
    assert abs(rr - np.dot(r_new, r_new)) <= bound
    # fixed order: run to run the same bits
    assert rr == rr2 and np.array_equal(xo.view(np.uint64), x2.view(np.uint64))
    assert np.array_equal(ro.view(np.uint64), r2.view(np.uint64)) and np.array_equal(rold.view(np.uint64), rold2.view(np.uint64))


@pytest.mark.parametrize("n", SIZES)
def test_dot2_matches_numpy(n):
    rng = np.random.default_rng(9000 + n)
    r, rold, z = (rng.standard_normal(n) for _ in range(3))
    out, out2 = np.zeros(2), np.zeros(2)
    assert A.lib().sss_hip_host_dot2(n, dptr(r), dptr(rold), dptr(z), dptr(out)) == 0
    assert A.lib().sss_hip_host_dot2(n, dptr(r), dptr(rold), dptr(z), dptr(out2)) == 0
    for got, v in zip(out, (r, rold)):
        bound = 2 * _gamma(n) * np.dot(np.abs(v), np.abs(z))
        print(f"n={n}: |dot - numpy| / bound = {abs(got - np.dot(v, z)) / bound:.3f}")
        assert abs(got - np.dot(v, z)) <= bound
    assert np.array_equal(out, out2)


def test_entry_points_reject_bad_arguments():
    v = np.ones(4)
    assert A.lib().sss_hip_host_pcg_update(0, 1.0, 1.0, dptr(v), dptr(v), dptr(v), dptr(v), dptr(v), dptr(v)) == -12
    assert A.lib().sss_hip_host_dot2(4, dptr(v), dptr(v), None, dptr(v)) == -12
