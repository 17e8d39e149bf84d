"""What the tests of the coarse Krylov solve's routes share (CPU: test_coarse_routes_cpu.py, GPU:
test_gpu_coarse_routes.py): small inputs that send the reference CG (beta == 1 as compiled) and its
GMRES(30) fallback through every exit of their state machines, each with the route it is there for.

The inputs the other coarse tests use (random right-hand sides at tol 1e-7 from x0 = 0) take one route:
CG runs to maxit without a check firing, GMRES either converges in its first Krylov cycle or runs to
maxit (the table in test_coarse_routes_cpu.py).  The cases here reach the rest: check II (stagnation)
rewriting p once, a few times and up to ERROR_SOLVER_STAG, check III (false convergence) up to
ERROR_SOLVER_TOLSMALL, both checks ending the solve converged, the breakdown and SOLSTAG exits, the
immediate returns of both solvers, and GMRES's failed true-residual recheck and best-iterate restore.

A case is a named builder of (row_ptr, col_idx, val, b, x0) plus tol, row_cap and its route: the set of
oracle events (oracle.KRYLOV_EVENTS) that are non-zero, CG's status and GMRES's (None: GMRES must not
run).  The routes were measured on the CPU oracle (ora_krylov_events); test_coarse_routes_cpu.py pins
them there, so a route that moved shows on the host first.

Sizes: n in {1, 8, 63, 1024, 1025, 3000, 4096} give the register and one-launch CG forms one to four
entries per thread, a partial last wave and a partial last 128-entry chunk; 4097 takes the LDS-chunked
step; the long-row matrix has 2,600 rows.  Nothing is larger.  The two cases found by seed search use
numpy's Generator only (its streams are stable across versions); non-finite iterates are out of scope.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional

import numpy as np
import scipy.sparse as sp

#: rows up to which the register step and the one-launch CG run (kRegVec * kSeqBlock); past it every
#: form request runs the LDS-chunked step
REG_MAX_ROWS = 4096
FORMS = ("persist", "reg", "lds")
FORM_CODE = {"lds": 0, "reg": 1, "persist": 2}   # sss_hip_coarse_last's form field


class Case(NamedTuple):
    name: str
    n: int                         # rows
    build: Callable[[], tuple]     # -> (row_ptr, col_idx, val, b, x0)
    tol: float
    row_cap: int
    events: frozenset              # the oracle events that are non-zero, no other
    cg_status: int
    gm_status: Optional[int]       # None: CG's status is >= 0 and GMRES does not run


def csr_of(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M.indptr.astype(np.int32), M.indices.astype(np.int32), np.ascontiguousarray(M.data, dtype=np.float64)


def laplacian(n, diag, scale=1.0):
    """tridiag(-1, diag, -1) * scale; the 1 x 1 matrix for n = 1."""
    if n == 1:
        return sp.csr_matrix(np.array([[diag * scale]]))
    return sp.diags([-np.ones(n - 1), np.full(n, diag), -np.ones(n - 1)], [-1, 0, 1], format="csr") * scale


def long_row_matrix():
    """The matrix of test_gpu_parity.py::test_coarse_krylov_long_rows: 2,600 rows, the first 24 rows and
    columns dense (rows longer than a 2,048-entry tile).  Returns it with the generator that built it."""
    n, k = 2600, 24
    rng = np.random.default_rng(12)
    S = sp.random(n, n, density=6.0 / n, random_state=rng, format="csr")
    D = sp.lil_matrix((n, n))
    D[:k, :] = rng.uniform(-1.0, 1.0, (k, n))
    M = S + S.T + D + D.T
    M = (M + sp.diags(np.asarray(abs(M).sum(axis=1)).ravel() + 1.0)).tocsr()
    assert np.diff(M.indptr).max() > 2048
    return M, rng


def _normal(n, seed=None):
    return np.random.default_rng(n if seed is None else seed).standard_normal(n)


# ---------------------------------------------------------------- the builders
def _lap(n, diag, scale=1.0, b_scale=1.0):
    def build():
        return (*csr_of(laplacian(n, diag, scale)), _normal(n) * b_scale, np.zeros(n))
    return build


def _long(near):
    def build():
        M, rng = long_row_matrix()
        n = M.shape[0]
        if near:   # b = A 1, started a rounding error away from the solution
            return (*csr_of(M), M @ np.ones(n), 1.0 + 1e-9 * _normal(n, 5))
        return (*csr_of(M), rng.standard_normal(n), np.zeros(n))
    return build


def _tolsmall():
    """diag(uniform[0.5, 3]), n = 8: seed 43 is the first of default_rng(0, 1, ...) whose CG leaves by
    ERROR_SOLVER_TOLSMALL at tol 0.5."""
    rng = np.random.default_rng(43)
    d = rng.uniform(0.5, 3.0, 8)
    return (*csr_of(sp.diags(d, format="csr")), rng.standard_normal(8), np.zeros(8))


def _identity(n, c):
    def build():
        return (*csr_of(sp.identity(n, format="csr") * c), _normal(n), np.zeros(n))
    return build


def _stored_zero():
    rp, ci, v = csr_of(laplacian(63, 2.05))
    return rp, ci, np.zeros_like(v), _normal(63), np.zeros(63)


def _exact_start():
    M = laplacian(63, 2.05)
    return (*csr_of(M), M @ np.ones(63), np.ones(63))


def _zero_rhs(x0):
    def build():
        return (*csr_of(laplacian(63, 2.05)), np.zeros(63), np.full(63, x0))
    return build


def _skew():
    n = 100
    return (*csr_of(sp.diags([-np.ones(n - 1), np.ones(n - 1)], [-1, 1], format="csr")), _normal(n), np.zeros(n))


def _gmres_best():
    """Symmetric, n = 31, about 0.3 of the entries uniform[0, 1) (S + S^T) plus diag uniform[1, 4]: seed
    48 is the first whose CG runs to maxit and whose GMRES ends by copying x_best back, at tol 1e-4."""
    n = 31
    rng = np.random.default_rng(48)
    S = np.where(rng.random((n, n)) < 0.3, rng.random((n, n)), 0.0)
    M = S + S.T + np.diag(rng.uniform(1.0, 4.0, n))
    return (*csr_of(M), rng.standard_normal(n), np.zeros(n))


def _check2_converges():
    """2 I from x0 = 1e6: the first step is the solve, and |alpha| ||p|| / ||u|| ~ 1e-6 is below
    maxdiff = 0.5e-4, so check II fires and its recomputed residual meets the tolerance."""
    n = 8
    x0 = np.full(n, 1e6)
    return (*csr_of(sp.identity(n, format="csr") * 2.0), 2.0 * x0 + _normal(n), x0)


def _gmres_immediate():
    """1e25 I with ||b|| ~ 1e-26: ||r0|| / SMALLFLOAT is above the tolerance, the first CG step gives
    ||u||_inf ~ 1e-51 <= SMALLFLOAT (ERROR_SOLVER_SOLSTAG), and GMRES starts from a residual below
    tol * SMALLFLOAT: its immediate return."""
    n = 8
    return (*csr_of(sp.identity(n, format="csr") * 1e25), _normal(n) * 1e-26, np.zeros(n))


_STAG_EXIT = {"cg_check2", "cg_stag_inc", "cg_stag_exit"}
_STAG_ON = {"cg_check2", "cg_stag_inc", "cg_maxit"}
_GM_FIRST = {"gm_cycles", "gm_early_break"}                                   # converged in the first cycle
_GM_MAXIT = {"gm_cycles", "gm_early_break", "gm_recheck_failed", "gm_recombine", "gm_maxit"}
_BEST = {"cg_best_copied"}


def _case(name, n, build, tol, events, cg_status, gm_status, row_cap=0):
    return Case(name, n, build, tol, row_cap, frozenset(events), cg_status, gm_status)


CASES = [
    # check II fires 20 times in a row: p zeroed 19 times, then ERROR_SOLVER_STAG; GMRES converges
    _case("stag_exit_63", 63, _lap(63, 2.05), 0.5, _STAG_EXIT | _GM_FIRST, -42, 1),
    *[_case(f"stag_exit_{n}", n, _lap(n, 2.05), 0.5, _STAG_EXIT | _BEST | _GM_FIRST, -42, 3)
      for n in (1024, 1025, 3000, 4096, 4097)],
    # check II fires 8 / 1 / 1 / 3 / 1 times, p zeroed, and CG goes on to maxit
    *[_case(f"stag_on_{n}", n, _lap(n, 4.0), 1e-2, _STAG_ON | _BEST | _GM_FIRST, -48, 4)
      for n in (63, 1024, 3000, 4096, 4097)],
    _case("stag_exit_d4_1025", 1025, _lap(1025, 4.0), 1e-2, _STAG_EXIT | _BEST | _GM_FIRST, -42, 4),
    # check II on rows longer than a tile: the in-kernel residual sums them in k_resid's order
    _case("long_rows_tol1e-2", 2600, _long(False), 1e-2, _STAG_EXIT | _GM_FIRST, -42, 5),
    _case("long_rows_tol0.5", 2600, _long(False), 0.5, _STAG_EXIT | _GM_FIRST, -42, 1),
    # GMRES: 969 one-step Krylov cycles, each converged by its estimate and refuted by the true residual
    _case("long_rows_recheck", 2600, _long(True), 1e-7,
          _STAG_EXIT | _BEST | {"gm_cycles", "gm_early_break", "gm_recheck_failed", "gm_maxit"}, -42, -48),
    # the capped branch of the in-kernel residual
    _case("stag_exit_200_cap40", 200, _lap(200, 2.05), 0.5, _STAG_EXIT | _BEST | _GM_MAXIT, -42, -48, row_cap=40),
    # check III fires 30 times (and check II once): ERROR_SOLVER_TOLSMALL
    _case("tolsmall_8", 8, _tolsmall, 0.5,
          {"cg_check2", "cg_stag_inc", "cg_check3", "cg_more_step_inc", "cg_tolsmall_exit"} | _GM_FIRST, -44, 1),
    # true convergence at step 1 through check III: status >= 0, no GMRES
    _case("identity_100", 100, _identity(100, 3.0), 1e-7, {"cg_check3", "cg_check3_conv"}, 1, None),
    _case("identity_1", 1, _identity(1, 3.0), 1e-7, {"cg_check3", "cg_check3_conv"}, 1, None),
    # ... and through check II
    _case("check2_converges_8", 8, _check2_converges, 0.5, {"cg_check2", "cg_check2_conv"}, 1, None),
    # breakdown (|temp2| <= SMALLFLOAT2) at step 1: status >= 0, the best-so-far (zero) iterate restored
    _case("breakdown_tiny_63", 63, _lap(63, 2.05, scale=1e-200), 1e-7, {"cg_breakdown"} | _BEST, 1, None),
    _case("breakdown_zero_63", 63, _stored_zero, 1e-7, {"cg_breakdown"} | _BEST, 1, None),
    # ||u||_inf <= SMALLFLOAT: ERROR_SOLVER_SOLSTAG, then GMRES
    _case("solstag_63", 63, _lap(63, 2.05, scale=1e25, b_scale=1e-21), 1e-7,
          {"cg_solstag", "gm_cycles", "gm_early_break", "gm_recheck_failed", "gm_recombine"}, -43, 193),
    _case("solstag_gmres_immediate_8", 8, _gmres_immediate, 1e-7, {"cg_solstag", "gm_immediate"}, -43, 0),
    # immediate return: skip_restore, no step
    _case("immediate_exact_63", 63, _exact_start, 1e-7, {"cg_immediate"}, 0, None),
    _case("immediate_zero_63", 63, _zero_rhs(0.0), 1e-7, {"cg_immediate"}, 0, None),
    # normr0 from a non-zero start with b = 0
    _case("zero_rhs_x1_63", 63, _zero_rhs(1.0), 1e-7, {"cg_maxit"} | _BEST | _GM_MAXIT, -48, -48),
    # stagnation exit at the default tolerance, GMRES to maxit
    _case("skew_100", 100, _skew, 1e-7, _STAG_EXIT | _GM_MAXIT, -42, -48),
    # GMRES ends by copying x_best back
    _case("gmres_best_31", 31, _gmres_best, 1e-4, {"cg_maxit", "gm_best_copied"} | _BEST | _GM_MAXIT, -48, -48),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def forms_of(name):
    """The CG forms a case is run in: past REG_MAX_ROWS rows `persist` and `reg` run the LDS-chunked step
    themselves, so only `lds` is asked for there."""
    return ("lds",) if BY_NAME[name].n > REG_MAX_ROWS else FORMS


_built: dict = {}
_oracle: dict = {}


def inputs(name):
    """(row_ptr, col_idx, val, b, x0) of a case, built once; callers copy x0 and leave the rest alone."""
    if name not in _built:
        _built[name] = BY_NAME[name].build()
    return _built[name]


def run_oracle(name):
    """(x, route) of ora_coarest_solve on a case: route is oracle.krylov_events() right after it."""
    import ctypes as C

    import amg_amd as A
    import oracle
    from amg_amd._native import dptr

    c = BY_NAME[name]
    rp, ci, v, b, x0 = inputs(name)
    hold = A.NumpyCSR(rp, ci, v)
    x = x0.copy()
    oracle.load().ora_coarest_solve(C.byref(hold.mat), C.byref(A.SSS_VEC(len(b), dptr(b))),
                                    C.byref(A.SSS_VEC(len(x), dptr(x))), c.tol,
                                    C.byref(oracle.opts(row_cap=c.row_cap, verbose=0)))
    return x, oracle.krylov_events()


def oracle_result(name):
    """run_oracle(name), computed once and shared: callers leave x alone."""
    if name not in _oracle:
        _oracle[name] = run_oracle(name)
    return _oracle[name]
