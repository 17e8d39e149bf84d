"""GPU: the cycle and its smoothers at sweep counts other than SSS_amg_pars_init's 2 and 2.

pre_iter and post_iter are public fields of SSS_AMG_PARS.  With 2 sweeps a class of the no-copy
C/F-Jacobi and two-stage passes is written an even number of times whatever the inner step count, so
the closing copy back into x never runs; the divisor of the later sweeps (d_later) is used exactly
once; the exact smoother takes its fused two-sweep plan; and every branch on `post_iter > 0` or
`pre_iter > 0` (dead-F prolongation, fused C-row residual, pending F pass, zero-first pass) goes one
way.  The tests here run the same comparisons as the rest of the suite at 0, 1 and 3 sweeps:
bitwise against the CPU oracle wherever the summation order is the reference's, bitwise between the
engine's own forms (knob on/off, tail on/off, graph on/off), and to the free-order bounds of
test_gpu_free_order.py where it is not.

Hierarchies: 1138_bus, 7-pt 16^3 and 27-pt 10^3; 7-pt 24^3 and 27-pt 16^3 where the single-workgroup
tail has to engage.  The pairs and the helper that sets them are in sweep_cases.py.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import amg_amd as A
import oracle
from amg_amd._native import SSS_SMTR, dptr
from conftest import build_hierarchy, device_mode_oracle_opts, oracle_solve, vec
from sweep_cases import LEVEL_PAIRS, PAIRS, banded_csr, first_f_row_lacks_diagonal, sweeps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bus_h(bus_matrix, quiet):
    return build_hierarchy(bus_matrix, quiet)


@pytest.fixture(scope="module")
def p16_h(quiet):
    return build_hierarchy(A.generate(7, 16), quiet)


@pytest.fixture(scope="module")
def a10_h(quiet):
    return build_hierarchy(A.generate(27, 10), quiet)


@pytest.fixture(scope="module")
def p24_h(quiet):
    return build_hierarchy(A.generate(7, 24), quiet)


@pytest.fixture(scope="module")
def a16_h(quiet):
    return build_hierarchy(A.generate(27, 16), quiet)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _smtr(M, b, x, mark, nsweeps, post):
    s = SSS_SMTR()
    s.smoother = 2
    s.A = C.pointer(M)
    s.b = C.pointer(vec(b))
    s.x = C.pointer(vec(x))
    s.nsweeps = nsweeps
    s.istart, s.iend, s.istep = 0, M.num_rows - 1, -1 if post else 1
    s.cf_order = 1
    s.ordering = mark
    return s


def _oracle_smooth(L, b, x0, smoother, inner, nsweeps, post):
    """x after one oracle smoother call of `nsweeps` sweeps on level L, from x0"""
    ora = oracle.load()
    xr = x0.copy()
    if smoother == "jacobi" and inner > 0:
        ora.ora_cf_twostage(dptr(xr), C.byref(L.A), dptr(b), nsweeps, L.cfmark.d, inner)
    elif smoother == "jacobi":
        ora.ora_cf_jacobi(dptr(xr), C.byref(L.A), dptr(b), nsweeps, L.cfmark.d)
    else:
        s = _smtr(L.A, b, xr, L.cfmark.d, nsweeps, post)
        (ora.ora_smoother_post if post else ora.ora_smoother_pre)(C.byref(s))
    return xr


def _level_calls(H, levels, seed, **kw):
    """[(level, post, sweeps, b, x0, x_gpu)]: the device pre and post smoother of every level in `levels`
    on random (b, x), with the counts H carries now; b must come back untouched."""
    D = A.DeviceHierarchy(H, **kw)
    rng = np.random.default_rng(seed)
    out = []
    try:
        for l in levels:
            n = H.level(l).A.num_rows
            for post in (False, True):
                b = rng.standard_normal(n)
                x0 = rng.standard_normal(n)
                D.upload(l, "b", b)
                D.upload(l, "x", x0)
                D.smooth(l, post)
                xg = D.download(l, "x")
                assert _bits(D.download(l, "b"), b), (l, post)
                out.append((l, post, H.pars.post_iter if post else H.pars.pre_iter, b, x0, xg))
    finally:
        D.close()
    return out


MODES = [("exact", 0), ("jacobi", 0), ("jacobi", 1), ("jacobi", 2)]


def _check_level_smoothers(H, levels, smoother, inner, monkeypatch, what):
    for pre, post_n in LEVEL_PAIRS:
        with sweeps(H, pre, post_n):
            kw = dict(smoother=smoother, coarse="direct", relabel=1, inner=inner, inner_from=0)
            monkeypatch.setenv("SSS_HIP_NOCOPY", "1")
            calls = _level_calls(H, levels, 23, **kw)
            for l, post, ns, b, x0, xg in calls:
                where = (what, smoother, inner, (pre, post_n), l, post)
                if ns == 0:
                    assert _bits(xg, x0), where
                xr = _oracle_smooth(H.level(l), b, x0, smoother, inner, ns, post)
                assert np.isfinite(xr).all(), where
                assert _bits(xg, xr), (where, float(np.max(np.abs(xg - xr))))
            if smoother == "jacobi":   # the copy-per-pass form gives the no-copy form's values
                monkeypatch.setenv("SSS_HIP_NOCOPY", "0")
                again = _level_calls(H, levels, 23, **kw)
                for (l, post, *_, xg), (*_, xc) in zip(calls, again):
                    assert _bits(xg, xc), (what, smoother, inner, (pre, post_n), l, post, "NOCOPY=0")


@pytest.mark.parametrize("hname", ["bus_h", "p16_h", "a10_h"])
@pytest.mark.parametrize("smoother,inner", MODES)
def test_level_smoothers_bitwise(request, hname, smoother, inner, monkeypatch):
    """Every level's device pre and post smoother (GS-CF, C/F-Jacobi, two-stage with 1 and 2 inner
    steps) with 0, 1 and 3 sweeps in both directions, bitwise the oracle's with the same count; 0
    sweeps leave x as uploaded.  1 and 3 sweeps with inner 0 or 2 write each class an odd number of
    times, so the no-copy form ends in its copy back into x; SSS_HIP_NOCOPY=0 must give the same
    bits."""
    H = request.getfixturevalue(hname)
    _check_level_smoothers(H, range(H.num_levels - 1), smoother, inner, monkeypatch, hname)


@pytest.mark.parametrize("smoother,inner", MODES)
def test_banded_missing_diagonals_bitwise(quiet, smoother, inner, monkeypatch):
    """Level 0 = 600 banded rows, some without a diagonal and one storing 0.0.  GS-CF carries the
    divisor over such rows, from the end of one sweep into the next: sweep 0 divides by d_first,
    every later sweep by d_later, which 3 sweeps use twice and 1 sweep not at all.  The two arrays
    differ only where the first F rows lack a diagonal, as they do here (row 0).  The Jacobi forms
    leave all those rows as they are."""
    M = banded_csr()
    H = build_hierarchy(M.mat, quiet)
    assert H.num_levels >= 2 and H.level(0).A.num_rows == 600
    assert first_f_row_lacks_diagonal(H.level(0))   # or d_first and d_later would be the same array
    _check_level_smoothers(H, [0], smoother, inner, monkeypatch, "banded")
    del M


# ---------------------------------------------------------------- whole solves against the oracle
def _gpu_solve(H, max_it=100, **kw):
    n = H.level(0).A.num_rows
    D = A.DeviceHierarchy(H, **kw)
    try:
        D.upload(0, "b", np.ones(n))
        D.upload(0, "x", np.ones(n))
        rel = []
        for _ in range(max_it):
            D.cycle()
            rel.append(D.residual_norm() / np.sqrt(n))
            if rel[-1] < H.pars.tol:
                break
        return np.array(rel), D.download(0, "x")
    finally:
        D.close()


def _oracle_hist(H, **kw):
    n = H.level(0).A.num_rows
    x = np.ones(n)
    rtn, rel, _ = oracle_solve(H, np.ones(n), x, **kw)
    assert rtn.nits < 100 and np.isfinite(x).all()
    return rel, x


@pytest.mark.parametrize("hname", ["bus_h", "p16_h", "a10_h"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_solve_parity_mode(request, hname, pair):
    """Exact GS-CF and the reference's Krylov coarse solve: the oracle's iteration count, x bitwise,
    per-iteration relres to 1e-13 (the level-0 norm is a tree reduction on the GPU).  The exact
    smoother's fused plan is built for 2 sweeps; any other count takes the per-pass engines, here
    inside the cycle, with the zeroed iterate of the coarse levels."""
    H = request.getfixturevalue(hname)
    with sweeps(H, *pair):
        rel_r, x_r = _oracle_hist(H)
        rel_g, x_g = _gpu_solve(H, smoother="exact", coarse="krylov")
    assert len(rel_g) == len(rel_r), (rel_g, rel_r)
    assert _bits(x_g, x_r), float(np.max(np.abs(x_g - x_r)))
    assert np.allclose(rel_g, rel_r, rtol=1e-13, atol=0)


HYBRID = [(h, i, f, p) for h in ["p16_h", "a10_h"] for (i, f) in [(0, 2), (1, 1), (2, 1)]
          for p in [(1, 1), (1, 3), (0, 2), (2, 0)]] + [("bus_h", 1, 1, (1, 1)), ("bus_h", 1, 1, (3, 1))]


@pytest.mark.parametrize("hname,inner,inner_from,pair", HYBRID,
                         ids=lambda v: f"{v[0]}-{v[1]}" if isinstance(v, tuple) else None)
def test_solve_hybrid_krylov_bitwise(request, hname, inner, inner_from, pair):
    """Throughput smoothers (exact level 0 where it is chain-free, C/F-Jacobi, two-stage from
    inner_from) with the reference coarse solver: x bitwise the oracle's in the same per-level
    configuration.  Odd counts with inner 0 or 2 end each no-copy call in the copy back into x, whose
    result the residual, the restriction and the prolongation then read."""
    H = request.getfixturevalue(hname)
    kw = device_mode_oracle_opts(H, smoother="hybrid", coarse="krylov", inner=inner, inner_from=inner_from)
    with sweeps(H, *pair):
        rel_r, x_r = _oracle_hist(H, **kw)
        rel_g, x_g = _gpu_solve(H, smoother="hybrid", coarse="krylov", inner=inner, inner_from=inner_from)
    assert len(rel_g) == len(rel_r), (rel_g, rel_r)
    assert _bits(x_g, x_r), float(np.max(np.abs(x_g - x_r)))
    assert np.allclose(rel_g, rel_r, rtol=1e-13, atol=0)


@pytest.mark.parametrize("hname", ["bus_h", "p16_h"])
@pytest.mark.parametrize("pair", [(1, 1), (1, 2)], ids=lambda p: f"{p[0]}-{p[1]}")
def test_w_cycle_bitwise(request, hname, pair):
    """cycle_type = 2: a level re-descended after its post-smoother starts its pre-smoother from that
    iterate -- x bitwise the oracle's W-cycle."""
    H = request.getfixturevalue(hname)
    H.mg.pars.cycle_type = 2
    try:
        with sweeps(H, *pair):
            rel_r, x_r = _oracle_hist(H)
            rel_g, x_g = _gpu_solve(H, max_it=len(rel_r), smoother="exact", coarse="krylov")
    finally:
        H.mg.pars.cycle_type = 1
    assert len(rel_g) == len(rel_r)
    assert _bits(x_g, x_r), float(np.max(np.abs(x_g - x_r)))
    assert np.allclose(rel_g, rel_r, rtol=1e-13, atol=0)


def test_drop_in_solver_amg(bus_matrix, bus_h, capfd):
    """SSS_solver_amg through the C ABI with pre_iter = 1 and post_iter = 3 in the caller's
    parameters: the oracle's iteration count, x within 1e-10 relative of the oracle's."""
    n = bus_matrix.num_rows
    b, x = np.ones(n), np.ones(n)
    pars = A.default_pars()
    pars.pre_iter, pars.post_iter = 1, 3
    rtn = A.lib().SSS_solver_amg(C.byref(bus_matrix), C.byref(vec(x)), C.byref(vec(b)), C.byref(pars))
    C.CDLL(None).fflush(None)
    capfd.readouterr()
    with sweeps(bus_h, 1, 3):
        rel_r, x_r = _oracle_hist(bus_h)
    assert rtn.nits == len(rel_r)
    assert np.linalg.norm(x - x_r) <= 1e-10 * np.linalg.norm(x_r)


# ---------------------------------------------------------------- the engine's forms against each other
def _cycles(H, ncyc, **kw):
    """(residual norms, x, wp, ledger total, first tail level) after ncyc cycles from b = x = 1"""
    n = H.level(0).A.num_rows
    D = A.DeviceHierarchy(H, **kw)
    try:
        D.upload(0, "b", np.ones(n))
        D.upload(0, "x", np.ones(n))
        norms = []
        for _ in range(ncyc):
            D.cycle()
            norms.append(D.residual_norm())
        return (np.array(norms), D.download(0, "x"), D.download(0, "wp"), D.cycle_bytes()["total"],
                A.lib().sss_hip_tail_from(D.h))
    finally:
        D.close()


ELIM_PAIRS = [(1, 1), (1, 3), (3, 1), (0, 2), (2, 0)]

#: (knob, mode) -> the pairs at which the knob changes what one outer iteration streams, by the
#: conditions in the code (see test_eliminations_neutral)
_ANY = lambda pre, post: True          # noqa: E731
_POST = lambda pre, post: post > 0     # noqa: E731
_PRE = lambda pre, post: pre > 0       # noqa: E731
LEDGER_MOVES = {
    ("SSS_HIP_FUSE_RESID", "exact"): _ANY, ("SSS_HIP_FUSE_RESID", "hybrid"): _ANY,
    ("SSS_HIP_DEAD_PROLONG", "exact"): _POST, ("SSS_HIP_DEAD_PROLONG", "hybrid"): _POST,
    ("SSS_HIP_TILE_DIAG", "hybrid"): _ANY,
    ("SSS_HIP_PEND_F", "exact"): lambda pre, post: pre > 0 and post > 0,
    ("SSS_HIP_PEND_F", "hybrid"): lambda pre, post: pre > 0 and post > 0,
    ("SSS_HIP_ZERO_FIRST", "hybrid"): _PRE,
    ("SSS_HIP_INJECT", "exact"): _POST, ("SSS_HIP_INJECT", "hybrid"): _POST,
    ("SSS_HIP_NOCOPY", "hybrid"): _ANY,
}


@pytest.mark.parametrize("knob", ["SSS_HIP_FUSE_RESID", "SSS_HIP_DEAD_PROLONG", "SSS_HIP_TILE_DIAG", "SSS_HIP_PEND_F",
                                  "SSS_HIP_ZERO_FIRST", "SSS_HIP_INJECT", "SSS_HIP_NOCOPY"])
@pytest.mark.parametrize("smoother,coarse", [("exact", "krylov"), ("hybrid", "direct")])
def test_eliminations_neutral(p16_h, smoother, coarse, knob, monkeypatch):
    """7-pt 16^3, level 0 red-black.  Each exact elimination on and off (what each does:
    test_gpu_parity.py test_fused_residual_bitwise; SSS_HIP_NOCOPY: test_nocopy_jacobi_bitwise), at
    sweep counts on both sides of the conditions the cycle puts on them: over 4 cycles the residual
    norms, x and the in-cycle residual wp are bitwise identical.

    That a knob engaged shows in the byte ledger (sss_hip_cycle_bytes), whose total then differs
    between on and off.  Asserted where the code keeps the feature on: the fused C-row residual in
    any smoother call with a sweep (the descent's with pre_iter > 0, the outer one with
    post_iter > 0); the dead-F prolongation and its injection form with post_iter > 0; the staged
    diagonal in any tile pass of the hybrid mode; the pending F pass with post_iter > 0 (the C rows of the outer
    residual are then ready, and its F half computes the pass) and pre_iter > 0 (the cycle takes it);
    the zero-first pass on the C/F-Jacobi levels of the hybrid mode with pre_iter > 0; the no-copy
    form on those levels with any sweep.  The exact mode has no C/F-Jacobi level, so
    SSS_HIP_ZERO_FIRST and SSS_HIP_NOCOPY change nothing there and nothing is asserted of the
    ledger.  Nor for SSS_HIP_TILE_DIAG there: the exact mode's mirror keeps plain tiles (formats
    "lean"), which stage no diagonal, and the ledger total was measured equal with the knob on and
    off at every pair (6,078,726 B at (1, 3) both ways)."""
    H = p16_h
    moves = LEDGER_MOVES.get((knob, smoother))
    still = []
    for pair in ELIM_PAIRS:
        with sweeps(H, *pair):
            out = []
            for on in ("1", "0"):
                monkeypatch.setenv(knob, on)
                out.append(_cycles(H, 4, smoother=smoother, coarse=coarse))
        (n1, x1, w1, b1, _), (n0, x0, w0, b0, _) = out
        print(f"ledger {knob} {smoother} {pair}: on {b1:.0f} off {b0:.0f}")
        assert _bits(n1, n0), (pair, n1, n0)
        assert _bits(x1, x0), pair
        assert _bits(w1, w0), pair
        assert np.isfinite(n1).all() and n1[-1] < n1[0], (pair, n1)
        if moves is not None and moves(*pair) and b1 == b0:
            still.append((pair, b1))
    assert not still, (knob, smoother, still)


@pytest.mark.parametrize("smoother,coarse", [("exact", "krylov"), ("hybrid", "direct")])
def test_graph_replay_neutral(p16_h, smoother, coarse):
    """The captured cycle (the graph with and without the pending F pass, the residual graphs)
    replays what the eager launches compute, at every pair."""
    for pair in ELIM_PAIRS:
        with sweeps(p16_h, *pair):
            n1, x1, w1, *_ = _cycles(p16_h, 4, smoother=smoother, coarse=coarse, graph=1)
            n0, x0, w0, *_ = _cycles(p16_h, 4, smoother=smoother, coarse=coarse, graph=0)
        assert _bits(n1, n0), (pair, n1, n0)
        assert _bits(x1, x0), pair
        assert _bits(w1, w0), pair


@pytest.mark.parametrize("hname", ["p24_h", "a16_h"])
@pytest.mark.parametrize("inner", [1, 2])
def test_tail_bitwise(request, hname, inner, monkeypatch):
    """The coarse levels as one single-workgroup launch take their sweep counts from the parameters
    (TailLevel::pre, post): 4 cycles with SSS_HIP_TAIL=1 and 0 give the same norms and x bit for
    bit.  Odd counts with inner = 2 write each class an odd number of times and end tail_smooth in
    its copy back into x."""
    H = request.getfixturevalue(hname)
    monkeypatch.setenv("SSS_HIP_TAIL_NNZ", "1000000")
    kw = dict(smoother="hybrid", coarse="direct", sum_order=1, inner=inner, inner_from=1)
    for pair in ELIM_PAIRS:
        with sweeps(H, *pair):
            monkeypatch.setenv("SSS_HIP_TAIL", "1")
            n1, x1, _, _, from1 = _cycles(H, 4, **kw)
            monkeypatch.setenv("SSS_HIP_TAIL", "0")
            n0, x0, _, _, from0 = _cycles(H, 4, **kw)
        assert from1 > 0, (hname, pair, from1)
        assert from0 <= 0, (hname, pair, from0)
        assert _bits(n1, n0), (pair, n1, n0)
        assert _bits(x1, x0), (pair, float(np.max(np.abs(x1 - x0))))
        assert np.isfinite(n1).all() and n1[-1] < n1[0], (pair, n1)


# ---------------------------------------------------------------- free summation order
@pytest.fixture(params=["wave", "merged4"])
def all_wave(request, monkeypatch):
    """every matrix on the free-order kernels (test_gpu_free_order.py): a wave per row, or merged
    groups of 4 rows"""
    monkeypatch.setenv("SSS_HIP_WAVE_MIN", "1")
    monkeypatch.setenv("SSS_HIP_FREE_MIN", "1")
    if request.param == "wave":
        monkeypatch.setenv("SSS_HIP_MERGE_MIN_ROWS", str(1 << 30))
    else:
        monkeypatch.setenv("SSS_HIP_MERGE_MIN_ROWS", "1")
        monkeypatch.setenv("SSS_HIP_MERGE_G", "4")
        monkeypatch.setenv("SSS_HIP_MERGE_W", "4")
    return request.param


@pytest.mark.parametrize("hname", ["p16_h", "a10_h"])
@pytest.mark.parametrize("inner", [0, 1, 2])
def test_free_order_smoothers_close(request, hname, inner, all_wave):
    """One smoother call per level in the free order, 1 and 3 sweeps in both directions: within
    1e-12 relative of the oracle (test_gpu_free_order.py's bound for one call, unchanged)."""
    H = request.getfixturevalue(hname)
    for pair in [(1, 3), (3, 1)]:
        with sweeps(H, *pair):
            calls = _level_calls(H, range(H.num_levels - 1), 5, smoother="jacobi", coarse="direct", relabel=1,
                                 inner=inner, inner_from=0, sum_order=1)
        for l, post, ns, b, x0, xg in calls:
            xr = _oracle_smooth(H.level(l), b, x0, "jacobi", inner, ns, post)
            err = np.linalg.norm(xg - xr) / np.linalg.norm(xr)
            print(f"free-order call {hname} {all_wave} inner {inner} {pair} level {l} post {post}: {err:.3e}")
            assert err <= 1e-12, (pair, l, post, err)


@pytest.mark.parametrize("hname", ["p16_h", "a10_h"])
def test_free_order_cycles(request, hname, all_wave):
    """3 cycles of the throughput mode in the free and in the stored order: x within 1e-10 relative,
    the residual norms within 1e-8 (test_gpu_free_order.py's bounds, unchanged); two free-order runs
    bitwise identical."""
    H = request.getfixturevalue(hname)
    for pair in [(1, 1), (1, 3)]:
        with sweeps(H, *pair):
            n_s, x_s, *_ = _cycles(H, 3, smoother="hybrid", coarse="direct", sum_order=0)
            n_f, x_f, *_ = _cycles(H, 3, smoother="hybrid", coarse="direct", sum_order=1)
            n_2, x_2, *_ = _cycles(H, 3, smoother="hybrid", coarse="direct", sum_order=1)
        dx = np.linalg.norm(x_f - x_s) / np.linalg.norm(x_s)
        print(f"free-order cycles {hname} {all_wave} {pair}: dx {dx:.3e} dnorm {np.max(np.abs(n_f / n_s - 1)):.3e}")
        assert dx <= 1e-10, (pair, dx)
        assert np.allclose(n_f, n_s, rtol=1e-8, atol=0), (pair, n_f, n_s)
        assert _bits(x_f, x_2) and _bits(n_f, n_2), pair
