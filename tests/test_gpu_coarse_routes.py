"""GPU: every exit of the coarse CG and GMRES, in every CG form, bitwise the oracle's.

sss_coarse_krylov.hip holds three device forms of the reference CG, each with its own copy of the step's
state machine: `persist` (k_cg_persist, the whole loop in one launch, with its speculative p_{k+1} and
the rollback when check II or III rewrites p), `reg` (k_cg_step_reg with its in-kernel residual) and
`lds` (k_cg_step + k_resid gate 1 + k_cg_fix); the GMRES is steered by the host.  The cases of
coarse_route_cases.py send the reference through every branch (test_coarse_routes_cpu.py proves that
on the host); here each case runs in each form and must give the oracle's x bit for bit AND the oracle's
route (sss_hip_coarse_last against ora_krylov_events: statuses, iter, iter_best, stag, more_step, whether
GMRES ran, its iterations and Krylov cycles), in the form that was asked for.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import amg_amd as A
import oracle
from amg_amd._native import SSS_VEC, dptr
from conftest import build_hierarchy, vec
from coarse_route_cases import BY_NAME, CASES, FORM_CODE, forms_of, inputs, oracle_result

pytestmark = pytest.mark.gpu

#: sss_hip_coarse_last field -> ora_krylov_events slot
SAME = {"cg_status": "cg_status", "cg_iter": "cg_iter", "cg_iter_best": "cg_iter_best", "cg_stag": "cg_stag",
        "cg_more_step": "cg_more_step", "gm_ran": "gm_ran", "gm_status": "gm_status", "gm_iter": "gm_iter",
        "gm_cycles": "gm_cycles"}


def _cg_form(mp, form):
    """As test_gpu_parity.py: persist = the one-launch CG, reg = register step + SpMV, lds = LDS-chunked."""
    mp.setenv("SSS_HIP_CG_REG", "0" if form == "lds" else "1")
    mp.setenv("SSS_HIP_CG_PERSIST", "1" if form == "persist" else "0")


def _solve_and_check(hold, name, form):
    """One sss_hip_host_coarse_solve of case `name` on the matrix object `hold`, held to the oracle."""
    c = BY_NAME[name]
    _, _, _, b, x0 = inputs(name)
    x_ref, route = oracle_result(name)
    xg = x0.copy()
    rc = A.lib().sss_hip_host_coarse_solve(C.byref(hold.mat), C.byref(vec(b)), C.byref(vec(xg)), c.tol, 0, c.row_cap)
    assert rc == 0
    last = A.coarse_last()
    print(name, form, last)
    assert np.array_equal(xg.view(np.uint64), x_ref.view(np.uint64)), (name, form, last, route)
    assert {f: last[f] for f in SAME} == {f: route[o] for f, o in SAME.items()}, (name, form)
    # the form that was asked for ran: no silent fall-back of the one-launch CG to two kernels a step
    assert last["form"] == FORM_CODE[form], (name, form, last["form"])


@pytest.mark.parametrize("name,form", [(c.name, f) for c in CASES for f in forms_of(c.name)])
def test_route_bitwise(name, form, monkeypatch):
    _cg_form(monkeypatch, form)
    rp, ci, v, _, _ = inputs(name)
    _solve_and_check(A.NumpyCSR(rp, ci, v), name, form)


def test_route_fields_need_a_completed_krylov_solve():
    """sss_hip_coarse_last(NULL) after the explicit-inverse coarse mode reports that there is no Krylov
    route, instead of the one before."""
    rp, ci, v, b, x0 = inputs("identity_100")
    hold = A.NumpyCSR(rp, ci, v)
    x = x0.copy()
    assert A.lib().sss_hip_host_coarse_solve(C.byref(hold.mat), C.byref(vec(b)), C.byref(vec(x)), 1e-7, 0, 0) == 0
    assert A.coarse_last()["cg_status"] == 1
    assert A.lib().sss_hip_host_coarse_solve(C.byref(hold.mat), C.byref(vec(b)), C.byref(vec(x)), 1e-7, 1, 0) == 0
    out = (C.c_int * len(A.COARSE_LAST_FIELDS))()
    assert A.lib().sss_hip_coarse_last(None, out, len(out)) < 0


def _matvec(rp, ci, v, x):
    import scipy.sparse as sp
    return sp.csr_matrix((v, ci, rp), shape=(len(rp) - 1, len(rp) - 1)) @ x


@pytest.mark.parametrize("form", ["persist", "reg", "lds"])
@pytest.mark.parametrize("firing,plain", [("stag_on_3000", "immediate"), ("stag_exit_1025", "plain")])
def test_reuse_after_a_fired_check(firing, plain, form, monkeypatch):
    """A check-firing solve, a plain one, and the check-firing one again on the same cached CoarseKrylov
    (the same matrix object and switches: the host cache keeps its device form): all three bitwise the
    oracle.  The one-launch form keeps its epoch, tags, tw and command ring between launches; a rollback
    (seq += 2, the workers redoing SpMV k + 1 from tw) must leave them fit for the next launch.  The
    plain solve in between is the same matrix with b = A 1 from x0 = 1 (CG's immediate return: the exit
    command alone goes out) or with another right-hand side at tol 1e-7 (CG to maxit, no check)."""
    _cg_form(monkeypatch, form)
    rp, ci, v, b, _ = inputs(firing)
    n = len(b)
    hold = A.NumpyCSR(rp, ci, v)
    A.lib().sss_hip_host_cache_clear()
    _solve_and_check(hold, firing, form)
    if plain == "immediate":
        b2, x2 = _matvec(rp, ci, v, np.ones(n)), np.ones(n)
    else:
        b2, x2 = np.random.default_rng(77).standard_normal(n), np.zeros(n)
    xg, xr = x2.copy(), x2.copy()
    assert A.lib().sss_hip_host_coarse_solve(C.byref(hold.mat), C.byref(vec(b2)), C.byref(vec(xg)), 1e-7, 0, 0) == 0
    last = A.coarse_last()
    oracle.load().ora_coarest_solve(C.byref(hold.mat), C.byref(vec(b2)), C.byref(vec(xr)), 1e-7,
                                    C.byref(oracle.opts(verbose=0)))
    route = oracle.krylov_events()
    assert np.array_equal(xg.view(np.uint64), xr.view(np.uint64))
    assert {f: last[f] for f in SAME} == {f: route[o] for f, o in SAME.items()}
    assert last["form"] == FORM_CODE[form] and last["cg_stag"] == 1
    assert last["cg_status"] == (0 if plain == "immediate" else -48)
    _solve_and_check(hold, firing, form)


# ---------------------------------------------------------------- inside the cycle
@pytest.fixture(scope="module")
def bus_h(bus_matrix, quiet):
    return build_hierarchy(bus_matrix, quiet)


@pytest.fixture(scope="module")
def p32_h(quiet):
    return build_hierarchy(A.generate(7, 32), quiet)


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("hname,ctol", [("bus_h", 0.5), ("p32_h", 0.1)])
def test_cycle_with_a_firing_coarse_check(request, hname, ctol, graph):
    """Three parity-mode V-cycles (exact smoother, Krylov coarse solve) whose coarse CG leaves by
    ERROR_SOLVER_STAG every cycle: x bitwise ora_cycle's, with and without the captured graph, and the
    hierarchy's route fields show the check.

    The cycle hands the coarse solve pars.ctol only while ctol <= pars.tol, and tol * 0.1 otherwise
    (SSS_amg_cycle; ora_cycle and coarse_tol restate it), so with the default tol = 1e-6 every ctol of
    {0.5, 0.1, 1e-2} gives the coarse solve the same 1e-7 as the default and no check fires (measured on
    the oracle).  pars.tol = 1.0 for these cycles lets ctol through; nothing else in a bare cycle reads
    tol.  Measured on the oracle with that: 1138_bus's coarsest matrix (59 rows) takes the STAG exit in
    all three cycles at ctol 0.5; 7-pt 32^3's (322 rows) converges through check III at step 1 at 0.5
    (stag stays 1), takes the STAG exit in all three cycles at 0.1, and runs to maxit at 1e-2: so 0.5
    for bus_h and 0.1 for p32_h."""
    H = request.getfixturevalue(hname)
    old = (H.mg.pars.ctol, H.mg.pars.tol)
    H.mg.pars.ctol, H.mg.pars.tol = ctol, 1.0
    H.pars.ctol, H.pars.tol = ctol, 1.0
    try:
        n = H.level(0).A.num_rows
        b, x_r = np.ones(n), np.ones(n)
        H.mg.cg[0].x = SSS_VEC(n, dptr(x_r))
        H.mg.cg[0].b = SSS_VEC(n, dptr(b))
        routes = []
        for _ in range(3):
            oracle.load().ora_cycle(C.byref(H.mg), C.byref(oracle.opts(verbose=0)))
            routes.append(oracle.krylov_events())
        assert all(r["cg_status"] == -42 and r["cg_stag"] == 20 for r in routes), routes
        D = A.DeviceHierarchy(H, smoother="exact", coarse="krylov", graph=graph)
        try:
            D.upload(0, "b", np.ones(n))
            D.upload(0, "x", np.ones(n))
            lasts = []
            for _ in range(3):
                D.cycle()
                D.sync()
                lasts.append(D.coarse_last())
            x_g = D.download(0, "x")
        finally:
            D.close()
        print(hname, ctol, graph, lasts)
        assert np.array_equal(x_g.view(np.uint64), x_r.view(np.uint64))
        for last, route in zip(lasts, routes):
            assert last["cg_stag"] > 1 or last["cg_status"] == -42
            assert {f: last[f] for f in SAME} == {f: route[o] for f, o in SAME.items()}
    finally:
        H.mg.pars.ctol, H.mg.pars.tol = old
        H.pars.ctol, H.pars.tol = old
