"""GPU tests of the AMG-preconditioned flexible GMRES (sss_hip_fgmres) and its fused multi-vector
orthogonalisation kernels (sss_fgmres.hip).

- sss_hip_host_orth (the device's CGS2 step on host data) against numpy, at shapes below one
  workgroup, not a multiple of the vector width, and across the register-block width of 8;
- the device solve against the numpy restatement (fgmres_restatement.py) whose preconditioner is the
  oracle's V-cycle in the same mode: iteration counts equal (under the margin rule there), histories
  within 1e-6, the true residual below tol;
- the point of the feature on a nonsymmetric operator: fewer iterations than the V-cycle loop, where
  PCG does not get to tol at all;
- edge cases, determinism, the engine state FGMRES leaves behind, and the SSS_HIP_OUTER drop-in.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import amg_amd as A
import oracle
from amg_amd._native import SSS_VEC, dptr
from conftest import device_mode_oracle_opts
from fgmres_restatement import TOL, assert_margin, cgs2, convdiff_hierarchy, oracle_fgmres, true_relres

pytestmark = pytest.mark.gpu

MODES = {   # engine mode -> oracle options of the same algorithm (None: read from the device's levels)
    "hybrid": (dict(smoother="hybrid", coarse="direct"), None),
    "exact": (dict(smoother="exact", coarse="krylov"), {}),
}
CASES = {"n11p2m20": (11, 2.0, 20), "n11p2m3": (11, 2.0, 3), "n16p2m20": (16, 2.0, 20), "n11p0m20": (11, 0.0, 20)}
U = 2.0 ** -53


@pytest.fixture(scope="module")
def hier(quiet):
    cache = {}

    def get(n, p):
        if (n, p) not in cache:
            cache[(n, p)] = convdiff_hierarchy(n, p, quiet)
        return cache[(n, p)][1]
    return get


@pytest.fixture(scope="module")
def restated(hier):
    """The restatement's (iterations, history, x), computed once per (mode, n, p, restart, maxit)."""
    cache, opts = {}, {}

    def get(mode, n, p, restart, maxit=100):
        key = (mode, n, p, restart, maxit)
        if key not in cache:
            H = hier(n, p)
            if (mode, n, p) not in opts:
                kw = MODES[mode][1]
                opts[(mode, n, p)] = kw if kw is not None else device_mode_oracle_opts(H, **MODES[mode][0])
            cache[key] = oracle_fgmres(H, oracle.opts(**opts[(mode, n, p)]), TOL, restart, maxit)
        return cache[key]
    return get


def _gpu_fgmres(H, mode, restart, maxit=100, b=None, x0=None, tol=TOL):
    n = H.level(0).A.num_rows
    D = A.DeviceHierarchy(H, **MODES[mode][0])
    D.upload(0, "b", np.ones(n) if b is None else b)
    D.upload(0, "x", np.zeros(n) if x0 is None else x0)
    its, hist = D.fgmres(tol, restart, maxit)
    x = D.download(0, "x")
    b_after = D.download(0, "b")
    D.close()
    assert np.array_equal(b_after, np.ones(n) if b is None else b)   # the right-hand side is restored
    return its, hist, x


# ---- the orthogonalisation kernels ----------------------------------------------------------
@pytest.mark.parametrize("k", [1, 7, 8, 9, 21])
@pytest.mark.parametrize("n", [1, 63, 1331, 4097])
def test_host_orth_matches_numpy_cgs2(n, k):
    """hcol within the reordered-summation bound 4 n u (|w| . |v_i|) of numpy's CGS2, and w within
    the bound that follows from it: w_out = w - V h up to the rounding of two k-term updates in each
    of the two implementations, so |dw_i| <= sum_c bound_h[c] |V_ic| + 4 (k + 2) u (|w_i| + (|V| |h|)_i).
    An orthonormal n x k basis needs k <= n: at n = 1 every k is the one-column case."""
    k = min(k, n)
    rng = np.random.default_rng(1000 * n + k)
    Q, _ = np.linalg.qr(rng.standard_normal((n, k)))
    V = np.ascontiguousarray(Q.T)   # k columns of n, back to back
    w_in = rng.standard_normal(n)
    h_ref, w_ref, nrm_ref = cgs2(V, w_in)
    outs = []
    for _ in range(2):
        w, h, nrm = w_in.copy(), np.zeros(k), np.zeros(1)
        assert A.lib().sss_hip_host_orth(n, k, dptr(V), dptr(w), dptr(h), dptr(nrm)) == 0
        outs.append((w, h, nrm[0]))
    (w, h, nrm), (w2, h2, nrm2) = outs
    assert np.array_equal(w.view(np.uint64), w2.view(np.uint64)) and np.array_equal(h, h2) and nrm == nrm2
    bound_h = 4 * n * U * (np.abs(V) @ np.abs(w_in))
    bound_w = bound_h @ np.abs(V) + 4 * (k + 2) * U * (np.abs(w_in) + np.abs(h_ref) @ np.abs(V))
    print(f"n={n} k={k}: max |dh|/bound {np.max(np.abs(h - h_ref) / bound_h):.3f}, "
          f"max |dw|/bound {np.max(np.abs(w - w_ref) / bound_w):.3f}, "
          f"|V^T w|/|w_in| {np.max(np.abs(V @ w)) / np.linalg.norm(w_in):.2e}")
    assert np.all(np.abs(h - h_ref) <= bound_h)
    assert np.all(np.abs(w - w_ref) <= bound_w)
    assert np.max(np.abs(V @ w)) <= 1e-13 * np.linalg.norm(w_in)
    assert abs(nrm - np.linalg.norm(w)) <= 4 * n * U * nrm + 1e-300
    assert abs(nrm - nrm_ref) <= np.linalg.norm(bound_w) + 4 * n * U * nrm_ref


# ---- the solve against the restatement ------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("mode", ["hybrid", "exact"])
def test_fgmres_matches_restatement(hier, restated, mode, case):
    n, p, restart = CASES[case]
    H = hier(n, p)
    its_r, hist_r, x_r = restated(mode, n, p, restart)
    assert_margin(hist_r, TOL, f"{mode} {case}")
    its, hist, x = _gpu_fgmres(H, mode, restart)
    print(f"{mode} {case}: {its} iterations (restatement {its_r}), estimates {hist}")
    assert its == its_r
    assert hist[-1] < TOL
    assert np.allclose(hist, hist_r, rtol=1e-6, atol=0)
    assert np.linalg.norm(x - x_r) <= 1e-6 * np.linalg.norm(x_r)
    assert true_relres(H, x) < TOL


@pytest.mark.parametrize("mode", ["hybrid", "exact"])
def test_fgmres_converges_where_pcg_cannot(hier, mode):
    """Nonsymmetric convection-diffusion 16^3, Peclet 2: FGMRES needs fewer iterations than the
    engine's own V-cycle loop, and PCG (which needs an SPD operator) is not at tol after 30."""
    H = hier(16, 2.0)
    n = H.level(0).A.num_rows
    its, hist, x = _gpu_fgmres(H, mode, 20)
    assert hist[-1] < TOL and true_relres(H, x) < TOL
    D = A.DeviceHierarchy(H, **MODES[mode][0])
    D.upload(0, "b", np.ones(n))
    D.upload(0, "x", np.zeros(n))
    cycles = 0
    while cycles < 100:
        D.cycle()
        cycles += 1
        if D.residual_norm() / np.sqrt(n) < TOL:
            break
    D.upload(0, "b", np.ones(n))
    D.upload(0, "x", np.zeros(n))
    its_cg, hist_cg = D.pcg(TOL, 30)
    D.close()
    print(f"{mode}: FGMRES {its}, V-cycle loop {cycles}, PCG {its_cg} (relres {hist_cg[-1]:.3e})")
    assert its < cycles
    assert its_cg == 30 and not hist_cg[-1] < TOL


# ---- edge cases on 11^3 ---------------------------------------------------------------------
def test_zero_rhs(hier):
    H = hier(11, 2.0)
    n = H.level(0).A.num_rows
    its, hist, x = _gpu_fgmres(H, "exact", 20, b=np.zeros(n), x0=np.ones(n))
    assert its == 0 and len(hist) == 0 and not x.any()


def test_exact_initial_guess(hier):
    """r0 = 0 exactly (b = A 1 in small integers, x0 = 1): no iteration, x untouched, no NaN."""
    H = hier(11, 2.0)
    A0 = H.level(0).A
    n = A0.num_rows
    b = np.zeros(n)
    oracle.load().ora_mv_mxy(C.byref(A0), dptr(np.ones(n)), dptr(b))
    its, hist, x = _gpu_fgmres(H, "exact", 20, b=b, x0=np.ones(n))
    assert its == 0 and np.array_equal(x, np.ones(n))


@pytest.mark.parametrize("mode", ["hybrid", "exact"])
def test_converged_initial_guess(hier, mode):
    H = hier(11, 2.0)
    _, _, x = _gpu_fgmres(H, mode, 20)
    its, hist, x2 = _gpu_fgmres(H, mode, 20, x0=x)
    assert its in (0, 1)
    assert np.all(np.isfinite(x2)) and np.all(np.isfinite(hist))
    assert true_relres(H, x2) < TOL


@pytest.mark.parametrize("mode", ["hybrid", "exact"])
def test_maxit_stops_with_the_columns_so_far(hier, restated, mode):
    H = hier(11, 2.0)
    its_r, hist_r, x_r = restated(mode, 11, 2.0, 20, 2)
    its, hist, x = _gpu_fgmres(H, mode, 20, maxit=2)
    assert its == its_r == 2
    assert np.allclose(hist, hist_r, rtol=1e-6, atol=0)
    assert np.linalg.norm(x - x_r) <= 1e-6 * np.linalg.norm(x_r)


def test_restart_one(hier, restated):
    """FGMRES(1): every iteration is a restart (k = 1 in every kernel); four of them, as restated."""
    H = hier(11, 2.0)
    its_r, hist_r, x_r = restated("exact", 11, 2.0, 1, 4)
    its, hist, x = _gpu_fgmres(H, "exact", 1, maxit=4)
    assert its == its_r == 4
    assert np.allclose(hist, hist_r, rtol=1e-6, atol=0)
    assert np.linalg.norm(x - x_r) <= 1e-6 * np.linalg.norm(x_r)


def test_hist_cap_one_and_bad_restart(hier):
    H = hier(11, 2.0)
    n = H.level(0).A.num_rows
    its_full, hist_full, x_full = _gpu_fgmres(H, "exact", 20)
    D = A.DeviceHierarchy(H, **MODES["exact"][0])
    D.upload(0, "b", np.ones(n))
    D.upload(0, "x", np.zeros(n))
    hist = np.full(3, -1.0)
    its, rel = C.c_int(), C.c_double()
    assert A.lib().sss_hip_fgmres(D.h, TOL, 20, 100, C.byref(its), C.byref(rel), dptr(hist), 1) == 0
    x = D.download(0, "x")
    assert its.value == its_full and rel.value == hist_full[-1]
    assert hist[0] == hist_full[0] and hist[1] == hist[2] == -1.0   # only hist_cap entries written
    assert np.array_equal(x.view(np.uint64), x_full.view(np.uint64))
    # restart < 1 is an input error (ERROR_INPUT_PAR = -12), through the binding too
    assert A.lib().sss_hip_fgmres(D.h, TOL, 0, 100, C.byref(its), C.byref(rel), None, 0) == -12
    with pytest.raises(RuntimeError):
        D.fgmres(TOL, restart=0)
    D.close()


@pytest.mark.parametrize("mode", ["hybrid", "exact"])
def test_deterministic(hier, mode):
    H = hier(11, 2.0)
    _, h1, x1 = _gpu_fgmres(H, mode, 3)
    _, h2, x2 = _gpu_fgmres(H, mode, 3)
    assert np.array_equal(x1.view(np.uint64), x2.view(np.uint64))
    assert np.array_equal(h1, h2)


@pytest.mark.parametrize("mode", ["hybrid", "exact"])
def test_engine_state_after_fgmres(hier, mode):
    """Cycles and residual norms right after fgmres equal those of a fresh hierarchy started from
    the same b and x: nothing stale is left of the cycle's fused residual halves."""
    H = hier(11, 2.0)
    n = H.level(0).A.num_rows

    def steps(D):
        out = []
        for _ in range(2):
            D.cycle()
            out.append(D.residual_norm())
        out.append(D.residual_norm())
        return out, D.download(0, "x")

    D = A.DeviceHierarchy(H, **MODES[mode][0])
    D.upload(0, "b", np.ones(n))
    D.upload(0, "x", np.zeros(n))
    D.cycle()
    D.residual_norm()   # leaves the engine's carried state set, as a solve loop would
    D.fgmres(TOL, 3, 4)
    x_mid = D.download(0, "x")
    res, x = steps(D)
    D.close()
    F = A.DeviceHierarchy(H, **MODES[mode][0])
    F.upload(0, "b", np.ones(n))
    F.upload(0, "x", x_mid)
    res_f, x_f = steps(F)
    F.close()
    assert res == res_f
    assert np.array_equal(x.view(np.uint64), x_f.view(np.uint64))


# ---- the drop-in ----------------------------------------------------------------------------
def _dropin_solve(H, quiet):
    n = H.level(0).A.num_rows
    x, b = np.zeros(n), np.ones(n)
    with quiet():
        rtn = A.lib().SSS_amg_solve(C.byref(H.mg), C.byref(SSS_VEC(n, dptr(x))), C.byref(SSS_VEC(n, dptr(b))))
    return rtn, x


def test_dropin_outer_fgmres(quiet, monkeypatch):
    _, H = convdiff_hierarchy(11, 2.0, quiet)
    n = H.level(0).A.num_rows
    monkeypatch.setenv("SSS_HIP_OUTER", "fgmres:3")
    rtn, x = _dropin_solve(H, quiet)
    assert rtn.nits == 5 and rtn.rres < H.pars.tol
    assert abs(rtn.rres - true_relres(H, x)) <= 1e-6 * rtn.rres
    its, hist, x_d = _gpu_fgmres(H, "exact", 3, maxit=H.pars.max_it, tol=H.pars.tol)
    assert its == 5
    assert np.array_equal(x.view(np.uint64), x_d.view(np.uint64))
    # the residual of the returned x is in the level-0 work vector, as after the V-cycle loop
    r = np.ctypeslib.as_array(H.mg.cg[0].wp.d, shape=(n,))
    assert abs(np.linalg.norm(r) - rtn.ares) <= 1e-12 * rtn.ares


def test_dropin_unset_is_the_vcycle_loop(quiet, monkeypatch):
    _, H = convdiff_hierarchy(11, 2.0, quiet)
    n = H.level(0).A.num_rows
    monkeypatch.delenv("SSS_HIP_OUTER", raising=False)
    rtn, x = _dropin_solve(H, quiet)
    D = A.DeviceHierarchy(H)
    D.upload(0, "b", np.ones(n))
    D.upload(0, "x", np.zeros(n))
    rel = []
    while len(rel) < H.pars.max_it:
        D.cycle()
        rel.append(D.residual_norm() / np.sqrt(n))
        if rel[-1] < H.pars.tol:
            break
    x_d = D.download(0, "x")
    D.close()
    assert rtn.nits == len(rel) and rtn.rres == rel[-1]
    assert np.array_equal(x.view(np.uint64), x_d.view(np.uint64))
