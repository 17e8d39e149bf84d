"""numpy restatement of the engine's AMG-preconditioned flexible GMRES (sss_hip_fgmres), for the
tests: right-preconditioned FGMRES(m) with classical Gram-Schmidt applied twice, M^-1 = one oracle
V-cycle (ora_cycle) on (r, 0), A x = ora_mv_mxy, Givens rotations, the same stopping rule (the
estimate |g_{j+1}| / ||b|| < tol, or maxit iterations in total) and the same restart.  Structured
like _oracle_pcg in test_gpu_pcg.py.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import amg_amd as A
import oracle
from amg_amd._native import SSS_VEC, dptr

TOL = 1e-6


def convdiff_hierarchy(n: int, p: float, quiet_cls):
    """(matrix holder, Hierarchy) of convdiff_csr(n, p); the holder keeps the numpy arrays alive."""
    M = A.convdiff_csr(n, p)
    with quiet_cls():
        return M, A.Hierarchy(M.mat)


def cgs2(V: np.ndarray, w: np.ndarray):
    """w against the rows of V by classical Gram-Schmidt applied twice: (h, w_out, ||w_out||)."""
    c1 = V @ w
    w = w - c1 @ V
    c2 = V @ w
    w = w - c2 @ V
    return c1 + c2, w, float(np.linalg.norm(w))


def oracle_fgmres(H, o, tol, restart, maxit=100, b=None, x0=None):
    """(iterations, history of the estimate, x) of FGMRES(restart) on level 0 of H with the oracle's
    V-cycle under options o as the preconditioner."""
    ora = oracle.load()
    A0 = H.level(0).A
    n = A0.num_rows
    bvec, xv = np.zeros(n), np.zeros(n)
    H.mg.cg[0].b = SSS_VEC(n, dptr(bvec))
    H.mg.cg[0].x = SSS_VEC(n, dptr(xv))

    def M(r):
        bvec[:] = r
        xv[:] = 0.0
        ora.ora_cycle(C.byref(H.mg), C.byref(o))
        return xv.copy()

    def Ax(v):
        y = np.zeros(n)
        ora.ora_mv_mxy(C.byref(A0), dptr(np.ascontiguousarray(v)), dptr(y))
        return y

    b = np.ones(n) if b is None else np.array(b, dtype=np.float64)
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    nb = np.linalg.norm(b)
    hist = []
    if nb == 0.0:
        return 0, np.array(hist), np.zeros(n)
    m = min(restart, max(maxit, 1))
    done = maxit < 1
    while not done:
        r = b - Ax(x)
        beta = np.linalg.norm(r)
        if beta == 0.0:
            break
        V = np.zeros((m + 1, n))
        Z = np.zeros((m, n))
        R = np.zeros((m + 1, m))
        cs, sn, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        V[0] = r / beta
        g[0] = beta
        k = 0
        for j in range(m):
            Z[j] = M(V[j])
            h, w, nw = cgs2(V[: j + 1], Ax(Z[j]))
            col = np.append(h, nw)
            for i in range(j):
                col[i], col[i + 1] = cs[i] * col[i] + sn[i] * col[i + 1], -sn[i] * col[i] + cs[i] * col[i + 1]
            d = np.hypot(col[j], col[j + 1])
            cs[j], sn[j] = (col[j] / d, col[j + 1] / d) if d != 0.0 else (1.0, 0.0)
            col[j], col[j + 1] = d, 0.0
            R[: j + 2, j] = col
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            hist.append(abs(g[j + 1]) / nb)
            k = j + 1
            if nw != 0.0:
                V[j + 1] = w / nw
            done = hist[-1] < tol or len(hist) >= maxit or nw == 0.0
            if done:
                break
        y = np.linalg.solve(np.triu(R[:k, :k]), g[:k])
        x = x + y @ Z[:k]
    return len(hist), np.array(hist), x


def assert_margin(hist, tol, what):
    """A case whose iteration count a test compares must not sit where rounding could move the
    count: the last estimate at most 0.95 tol, the one before it at least 1.05 tol."""
    prev = hist[-2] if len(hist) > 1 else 1.0
    assert hist[-1] <= 0.95 * tol and prev >= 1.05 * tol, (
        f"{what}: the restatement's last estimates {prev:.3e}, {hist[-1]:.3e} are within 5% of tol {tol:g}; "
        "pick another input for this test")


def true_relres(H, x, b=None):
    A0 = H.level(0).A
    n = A0.num_rows
    b = np.ones(n) if b is None else b
    y = np.zeros(n)
    oracle.load().ora_mv_mxy(C.byref(A0), dptr(np.ascontiguousarray(x)), dptr(y))
    return float(np.linalg.norm(b - y) / np.linalg.norm(b))
