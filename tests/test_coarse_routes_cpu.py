"""CPU: the reference coarse solve alone takes the routes coarse_route_cases.py declares.

ora_krylov_events counts every branch of ora_cg and ora_gmres (counters only: the oracle's arithmetic
is unchanged, test_oracle.py and test_ref_units.py pin it).  For every case the non-zero events and both
statuses are exactly the declared route, and over all cases no event stays at zero; the GPU test
(test_gpu_coarse_routes.py) then holds every CG form to the same routes, bitwise.

What the coarse inputs of the other tests reach, measured with the same counters (tol 1e-7, x0 = 0;
test_existing_inputs_take_one_route re-measures the rows marked *):

  input                                               CG                    GMRES
  bus_h coarsest (59 rows), rng(9) b               *  maxit, best copied    maxit; 39 cycles, 6 rechecks failed
  bus_h coarsest, linspace b, row cap 0 / 40       *  maxit                 maxit; 36 / 35 cycles
  p32_h coarsest (322 rows), rng(9) b              *  maxit, best copied    converged in cycle 1 (12 steps)
  a27_h coarsest (145 rows), rng(9) b              *  maxit, best copied    converged in cycle 1 (12 steps)
  p32_h levels of 3,195 and 32,768 rows               maxit, best copied    cycle 1 (28 steps) / maxit
  step_sizes n = 1                                 *  check III converged   not run
  step_sizes n = 2, 17                             *  maxit, best copied    converged in cycle 1
  step_sizes n = 1024, 4095, 4096, 4097            *  maxit (best copied)   maxit; 34-35 cycles, 2 rechecks failed
  long_rows (2,600 rows)                              maxit                 converged in cycle 1 (21 steps)
  the coarse solves of 3 V-cycles on p32_h / bus_h    as the first rows     as the first rows

Never reached by them: breakdown, solstag, check II (entered, converged, STAG exit, stag++), check III
not converging (TOLSMALL exit, more_step++), CG's immediate return, GMRES's immediate return and GMRES's
x_best restore.  The only check that ever fires is check III converging at n = 1.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import amg_amd as A
import oracle
from amg_amd._native import SSS_KRYLOV
from conftest import build_hierarchy, vec
from coarse_route_cases import BY_NAME, CASES, csr_of, inputs, laplacian, oracle_result, run_oracle

#: the events none of the older coarse inputs reaches (the docstring's last paragraph)
NEW_EVENTS = {"cg_breakdown", "cg_solstag", "cg_check2", "cg_check2_conv", "cg_stag_exit", "cg_tolsmall_exit",
              "cg_stag_inc", "cg_more_step_inc", "cg_immediate", "gm_immediate", "gm_best_copied"}


def _nonzero_events(route):
    return {e for e in oracle.KRYLOV_EVENTS if route[e]}


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_oracle_takes_the_declared_route(name):
    c = BY_NAME[name]
    x, route = oracle_result(name)
    assert len(inputs(name)[3]) == c.n
    assert np.all(np.isfinite(x))
    assert _nonzero_events(route) == set(c.events), route
    assert route["cg_status"] == c.cg_status
    assert route["gm_ran"] == (c.gm_status is not None)
    assert route["gm_ran"] == (c.cg_status < 0)          # SSS_amg_coarest_solve's rule
    if c.gm_status is not None:
        assert route["gm_status"] == c.gm_status
    # the counters the device reports too (sss_hip_coarse_last) hang together with the events
    assert route["cg_stag"] == 1 + route["cg_stag_inc"] and route["cg_more_step"] == 1 + route["cg_more_step_inc"]


def test_every_event_is_reached():
    reached = set()
    for c in CASES:
        reached |= _nonzero_events(oracle_result(c.name)[1])
    assert reached == set(oracle.KRYLOV_EVENTS), set(oracle.KRYLOV_EVENTS) - reached


def test_accessor_is_per_call_and_bounded():
    """A later call replaces the route; fewer slots than there are can be asked for; ora_gmres on its own
    clears the CG slots."""
    _, first = run_oracle("stag_exit_63")
    assert first["cg_check2"] == 20 and first["cg_stag_exit"] == 1 and first["cg_stag_inc"] == 19
    _, second = run_oracle("identity_1")
    assert second["cg_check2"] == 0 and second["gm_ran"] == 0 and second["cg_check3_conv"] == 1
    run_oracle("stag_exit_63")
    out = (C.c_int * 4)(7, 7, 7, 7)
    oracle.load().ora_krylov_events(out, 3)
    assert list(out) == [0, 0, 20, 7]                    # breakdown, solstag, check II entered
    rp, ci, v, b, x0 = inputs("stag_exit_63")
    hold = A.NumpyCSR(rp, ci, v)
    x = x0.copy()
    bv, xv = vec(b), vec(x)
    ks = SSS_KRYLOV()
    ks.A, ks.b, ks.u = C.pointer(hold.mat), C.pointer(bv), C.pointer(xv)
    ks.tol, ks.matrix, ks.restart = 0.5, 1000, 30
    status = oracle.load().ora_gmres(C.byref(ks), 0)
    alone = oracle.krylov_events()
    assert alone["cg_check2"] == 0 and alone["cg_status"] == 0 and alone["cg_stag"] == 0
    assert alone["gm_ran"] == 1 and alone["gm_status"] == status and alone["gm_cycles"] >= 1


# ---------------------------------------------------------------- the premise, with the real fixtures
def _route(M, b, cap=0):
    x = np.zeros(len(b))
    oracle.load().ora_coarest_solve(C.byref(M), C.byref(vec(b)), C.byref(vec(x)), 1e-7,
                                    C.byref(oracle.opts(row_cap=cap, verbose=0)))
    return oracle.krylov_events()


def test_existing_inputs_take_one_route(bus_matrix, quiet):
    """The starred rows of the module docstring: no older coarse input reaches an event of NEW_EVENTS,
    and apart from n = 1 every one of them runs CG to maxit."""
    routes = {}
    for name, M in (("bus_h", bus_matrix), ("p32_h", A.generate(7, 32)), ("a27_h", A.generate(27, 16))):
        H = build_hierarchy(M, quiet)
        Lc = H.level(H.num_levels - 1)
        n = Lc.A.num_rows
        routes[name] = _route(Lc.A, np.random.default_rng(9).standard_normal(n))
        if name == "bus_h":
            for cap in (0, 40):
                routes[f"bus_h cap {cap}"] = _route(Lc.A, np.linspace(-1.0, 2.0, n), cap)
    for n in (1, 2, 17, 1024, 4095, 4096, 4097):
        hold = A.NumpyCSR(*csr_of(laplacian(n, 2.05)))
        routes[f"step_sizes {n}"] = _route(hold.mat, np.random.default_rng(n).standard_normal(n))
    for name, r in routes.items():
        assert not (_nonzero_events(r) & NEW_EVENTS), (name, r)
        if name == "step_sizes 1":
            assert r["cg_status"] == 1 and r["cg_check3_conv"] == 1 and not r["gm_ran"]
        else:
            assert r["cg_status"] == -48 and r["cg_maxit"] == 1 and r["cg_check3"] == 0 and r["gm_ran"], (name, r)
    assert routes["bus_h"]["gm_status"] == -48 and routes["p32_h"]["gm_status"] == 12
    assert routes["a27_h"]["gm_status"] == 12 and routes["step_sizes 4097"]["gm_status"] == -48
