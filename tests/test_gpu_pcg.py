"""GPU tests of the AMG-preconditioned CG (sss_hip_pcg; SURVEY.md §8f row 4, an engine extension).

Checks: convergence to tol with fewer iterations than the stand-alone V-cycle iteration, the true
residual ||b - A x|| / ||b|| (host, oracle SpMV) below tol, run-to-run determinism (bitwise x),
and agreement with a numpy restatement of the same flexible PCG whose preconditioner is the
oracle's V-cycle in the same mode (iteration counts equal, residual histories within 1e-6).

Stop-rule edges on 7-pt 11^3, as test_gpu_fgmres.py has them for FGMRES: a zero right-hand side, an
exact and a converged initial guess, maxit 3 and 0, hist_cap / NULL hist, a NaN in b, a NULL handle,
and the engine state a solve leaves behind.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import amg_amd as A
import oracle
from amg_amd._native import SSS_VEC, dptr
from conftest import build_hierarchy, device_mode_oracle_opts

pytestmark = pytest.mark.gpu

MODES = {   # engine mode -> oracle options of the same algorithm (None: read from the device's levels)
    "hybrid": (dict(smoother="hybrid", coarse="direct"), None),
    "exact": (dict(smoother="exact", coarse="krylov"), {}),
}


@pytest.fixture(scope="module")
def p32_h(quiet):
    return build_hierarchy(A.generate(7, 32), quiet)


@pytest.fixture(scope="module")
def a27_h(quiet):
    return build_hierarchy(A.generate(27, 16), quiet)


@pytest.fixture(scope="module")
def p11_h(quiet):
    return build_hierarchy(A.generate(7, 11), quiet)


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _gpu_pcg(H, mode, tol, maxit=100, b=None, x0=None):
    n = H.level(0).A.num_rows
    b = np.ones(n) if b is None else b
    D = A.DeviceHierarchy(H, **MODES[mode][0])
    D.upload(0, "b", b)
    D.upload(0, "x", np.zeros(n) if x0 is None else x0)
    its, hist = D.pcg(tol, maxit)
    x = D.download(0, "x")
    b_after = D.download(0, "b")
    D.close()
    assert np.array_equal(_u64(b_after), _u64(b))   # the right-hand side is restored
    return its, hist, x


def _raw_pcg(D, tol, maxit, hist=None, hist_cap=0):
    """sss_hip_pcg through ctypes: (return code, iterations, relres)."""
    its, rel = C.c_int(-1), C.c_double(-1.0)
    rc = A.lib().sss_hip_pcg(D.h, tol, maxit, C.byref(its), C.byref(rel), None if hist is None else dptr(hist), hist_cap)
    return rc, its.value, rel.value


def _true_relres(H, x, b):
    y = np.zeros(len(x))
    oracle.load().ora_mv_mxy(C.byref(H.level(0).A), dptr(x), dptr(y))
    return np.linalg.norm(b - y) / np.linalg.norm(b)


def _oracle_pcg(H, mode, tol, maxit=100):
    """numpy flexible CG (Polak-Ribiere), M^-1 = one oracle V-cycle on (r, 0)."""
    ora = oracle.load()
    kw = MODES[mode][1]
    o = oracle.opts(**(kw if kw is not None else device_mode_oracle_opts(H, **MODES[mode][0])))
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
        ora.ora_mv_mxy(C.byref(A0), dptr(v), dptr(y))
        return y

    b = np.ones(n)
    x = np.zeros(n)
    r = b - Ax(x)
    z = M(r)
    p = z.copy()
    rz = r @ z
    nb = np.linalg.norm(b)
    hist = []
    for _ in range(maxit):
        q = Ax(p)
        a = rz / (p @ q)
        x += a * p
        ro = r.copy()
        r -= a * q
        hist.append(np.linalg.norm(r) / nb)
        if hist[-1] < tol:
            break
        z = M(r)
        rzn = r @ z
        p = z + ((rzn - ro @ z) / rz) * p
        rz = rzn
    return len(hist), np.array(hist), x


@pytest.mark.parametrize("hname", ["p32_h", "a27_h"])
@pytest.mark.parametrize("mode", ["hybrid", "exact"])
def test_pcg_matches_restatement(request, hname, mode):
    H = request.getfixturevalue(hname)
    tol = H.pars.tol
    its, hist, x = _gpu_pcg(H, mode, tol)
    its_r, hist_r, x_r = _oracle_pcg(H, mode, tol)
    assert hist[-1] < tol
    assert its == its_r
    assert np.allclose(hist, hist_r, rtol=1e-6, atol=0)
    assert np.linalg.norm(x - x_r) <= 1e-6 * np.linalg.norm(x_r)


@pytest.mark.parametrize("mode", ["hybrid", "exact"])
def test_pcg_true_residual_and_speedup(p32_h, mode):
    H = p32_h
    A0 = H.level(0).A
    n = A0.num_rows
    its, hist, x = _gpu_pcg(H, mode, H.pars.tol)
    y = np.zeros(n)
    oracle.load().ora_mv_mxy(C.byref(A0), dptr(x), dptr(y))
    assert np.linalg.norm(np.ones(n) - y) / np.sqrt(n) < 10 * H.pars.tol
    # fewer iterations than the stand-alone V-cycle iteration of the same engine mode
    D = A.DeviceHierarchy(H, **MODES[mode][0])
    D.upload(0, "b", np.ones(n))
    D.upload(0, "x", np.zeros(n))
    cycles = 0
    while cycles < 100:
        D.cycle()
        cycles += 1
        if D.residual_norm() / np.sqrt(n) < H.pars.tol:
            break
    D.close()
    assert its < cycles


def test_pcg_deterministic(a27_h):
    _, h1, x1 = _gpu_pcg(a27_h, "hybrid", a27_h.pars.tol)
    _, h2, x2 = _gpu_pcg(a27_h, "hybrid", a27_h.pars.tol)
    assert np.array_equal(x1.view(np.uint64), x2.view(np.uint64))
    assert np.array_equal(h1, h2)


# ---- stop-rule edges on 11^3 ----------------------------------------------------------------
def test_zero_rhs(p11_h):
    n = p11_h.level(0).A.num_rows
    its, hist, x = _gpu_pcg(p11_h, "exact", p11_h.pars.tol, b=np.zeros(n), x0=np.ones(n))
    assert its == 0 and len(hist) == 0 and not x.any()


@pytest.mark.parametrize("mode", ["hybrid", "exact"])
def test_exact_initial_guess(p11_h, mode):
    """r0 = 0 exactly (b = A 1 in small integers, x0 = 1): z = 0 would give the step length 0 / 0 and a
    NaN iterate that never passes `rel < tol`; instead no iteration, relres 0, x untouched."""
    H = p11_h
    A0 = H.level(0).A
    n = A0.num_rows
    b = np.zeros(n)
    oracle.load().ora_mv_mxy(C.byref(A0), dptr(np.ones(n)), dptr(b))
    assert b.any()
    D = A.DeviceHierarchy(H, **MODES[mode][0])
    D.upload(0, "b", b)
    D.upload(0, "x", np.ones(n))
    hist = np.full(2, -1.0)
    rc, its, rel = _raw_pcg(D, H.pars.tol, 100, hist, 2)
    x, b_after = D.download(0, "x"), D.download(0, "b")
    D.close()
    assert rc == 0 and its == 0 and rel == 0.0
    assert np.array_equal(_u64(x), _u64(np.ones(n))) and np.array_equal(_u64(b_after), _u64(b))
    assert hist[0] == hist[1] == -1.0


@pytest.mark.parametrize("mode", ["hybrid", "exact"])
def test_converged_initial_guess(p11_h, mode):
    H = p11_h
    tol = H.pars.tol
    n = H.level(0).A.num_rows
    _, _, x = _gpu_pcg(H, mode, tol)
    its, hist, x2 = _gpu_pcg(H, mode, tol, x0=x)
    assert its in (0, 1)
    assert np.all(np.isfinite(x2)) and np.all(np.isfinite(hist))
    assert _true_relres(H, x2, np.ones(n)) < tol


@pytest.mark.parametrize("mode", ["hybrid", "exact"])
def test_maxit_three(p11_h, mode):
    H = p11_h
    tol = H.pars.tol
    its_full, hist_full, _ = _gpu_pcg(H, mode, tol)
    assert its_full >= 3   # hybrid: more than three, so maxit is what stops it
    its, hist, x = _gpu_pcg(H, mode, tol, maxit=3)
    its_r, hist_r, x_r = _oracle_pcg(H, mode, tol, maxit=3)
    assert its == its_r == 3
    assert np.array_equal(hist, hist_full[:3])   # bitwise the first three of the full run
    assert np.allclose(hist, hist_r, rtol=1e-6, atol=0)
    assert np.linalg.norm(x - x_r) <= 1e-6 * np.linalg.norm(x_r)


def test_maxit_zero(p11_h):
    n = p11_h.level(0).A.num_rows
    x0 = np.random.default_rng(5).standard_normal(n)
    its, hist, x = _gpu_pcg(p11_h, "exact", p11_h.pars.tol, maxit=0, x0=x0)
    assert its == 0 and len(hist) == 0
    assert np.array_equal(_u64(x), _u64(x0))


def test_hist_cap_one_and_null_hist(p11_h):
    H = p11_h
    tol = H.pars.tol
    n = H.level(0).A.num_rows
    its_full, hist_full, x_full = _gpu_pcg(H, "exact", tol)
    assert its_full > 1
    D = A.DeviceHierarchy(H, **MODES["exact"][0])
    for hist in (np.full(3, -1.0), None):
        D.upload(0, "b", np.ones(n))
        D.upload(0, "x", np.zeros(n))
        rc, its, rel = _raw_pcg(D, tol, 100, hist, 1 if hist is not None else 0)
        assert rc == 0 and its == its_full and rel == hist_full[-1]
        if hist is not None:   # only hist_cap entries are written
            assert hist[0] == hist_full[0] and hist[1] == hist[2] == -1.0
        assert np.array_equal(_u64(D.download(0, "x")), _u64(x_full))
    D.close()


@pytest.mark.parametrize("mode", ["hybrid", "exact"])
def test_nan_in_rhs(p11_h, mode):
    """One NaN in b: ERROR_SOLVER_EXIT at once (not maxit V-cycles on NaN vectors and return code 0),
    x the last finite iterate -- the initial guess -- and b back as it was."""
    H = p11_h
    n = H.level(0).A.num_rows
    b = np.ones(n)
    b[n // 2] = np.nan
    x0 = np.random.default_rng(6).standard_normal(n)
    D = A.DeviceHierarchy(H, **MODES[mode][0])
    D.upload(0, "b", b)
    D.upload(0, "x", x0)
    rc, its, _ = _raw_pcg(D, H.pars.tol, 100)
    x, b_after = D.download(0, "x"), D.download(0, "b")
    assert rc == -49 and its <= 1   # ERROR_SOLVER_EXIT
    assert np.array_equal(_u64(x), _u64(x0)) and np.array_equal(_u64(b_after), _u64(b))
    with pytest.raises(RuntimeError):
        D.pcg(H.pars.tol)
    D.close()


def test_null_handle():
    its, rel = C.c_int(), C.c_double()
    assert A.lib().sss_hip_pcg(None, 1e-8, 10, C.byref(its), C.byref(rel), None, 0) == -12   # ERROR_INPUT_PAR


@pytest.mark.parametrize("mode", ["hybrid", "exact"])
def test_engine_state_after_pcg(p11_h, mode):
    """One cycle on b = x = 1 right after a pcg is bitwise a fresh engine's."""
    H = p11_h
    n = H.level(0).A.num_rows
    out = []
    for solve_first in (True, False):
        D = A.DeviceHierarchy(H, **MODES[mode][0])
        if solve_first:
            D.upload(0, "b", np.ones(n))
            D.upload(0, "x", np.zeros(n))
            D.cycle()
            D.residual_norm()   # leaves the engine's carried state set, as a solve loop would
            D.pcg(H.pars.tol, 4)
        D.upload(0, "b", np.ones(n))
        D.upload(0, "x", np.ones(n))
        D.cycle()
        out.append((D.residual_norm(), D.download(0, "x")))
        D.close()
    assert out[0][0] == out[1][0]
    assert np.array_equal(_u64(out[0][1]), _u64(out[1][1]))
