"""CPU: aggressive PMIS coarsening (cs_type 4) and multipass interpolation (interp_type 4), engine
extensions, host side.  The distance-two graph, the final marks and the multipass P of
amg_amd/host/sss_setup.c are the plain-Python restatement of the rule (tests/mpass_cases.py), arrays equal
and values bit for bit, on the hand-built and the natural cases with both truncations; the invariants of the
split and of the weights; whole setups (fewer rows and a lower operator complexity than PMIS + interp 2,
SSS_SETUP_AGG_LEVELS, interp_type 4 after the other splits, convergence, the hierarchy file, the refresh);
the new symbols, the environment switches and the parameter print."""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import amg_amd as A
import mpass_cases as MP
import pmis_restatement as R
import refresh_cases as RC
from conftest import oracle_solve

ROOT = Path(__file__).resolve().parent.parent
CASES = MP.NATURAL + [f"p7_24_level{l}" for l in range(3)] + MP.HAND


def _host_split(c):
    """(m1, S2) of a case's S on the host."""
    m1 = A.pmis(*c.S)[0]
    return m1, A.agg_graph(*c.S, m1)


@pytest.mark.parametrize("name", CASES)
def test_host_graph_and_marks_equal_restatement(name, quiet):
    c = MP.all_cases(quiet)[name]
    want_mark, want_m1, want_s2 = MP.final_marks_restated(*c.S)
    with quiet():
        m1, s2 = _host_split(c)
        mark, ncoarse = A.pmis_agg(*c.S)
    assert np.array_equal(m1, want_m1), name
    MP.assert_same_graph(s2, want_s2, name)
    assert len(s2[0]) - 1 == (m1 == MP.CGPT).sum()
    assert np.array_equal(mark, want_mark) and ncoarse == (want_mark == MP.CGPT).sum(), name
    if name in MP.NATURAL or "_level" in name:
        assert np.array_equal(c.mark, want_mark), name   # what SSS_amg_coarsen left
    # the final C points are stage-one C points, and no two of them are mutual S2 neighbours
    assert (m1[mark == MP.CGPT] == MP.CGPT).all()
    cpts = np.flatnonzero(m1 == MP.CGPT)
    final_c = mark[cpts] == MP.CGPT
    rows = [set(s2[1][s2[0][r]:s2[0][r + 1]].tolist()) for r in range(len(cpts))]
    for r in np.flatnonzero(final_c):
        assert not any(final_c[q] and r in rows[q] for q in rows[r]), (name, r)


def test_hand_built_split_known_answer(quiet):
    """Point 0: a nonempty S2 row that nobody's S2 row names (lambda = 0): it becomes F.  Point 2: an empty
    S2 row: it stays C."""
    rp, ci = R.from_rows(MP.TWO_STAGE_S)
    with quiet():
        m1 = A.pmis(rp, ci)[0]
        s2 = A.agg_graph(rp, ci, m1)
        mark, ncoarse = A.pmis_agg(rp, ci)
    assert m1.tolist() == MP.TWO_STAGE_M1
    assert s2[0].tolist() == [0, 1, 1] and s2[1].tolist() == [1]
    assert mark.tolist() == MP.TWO_STAGE_FINAL and ncoarse == 1


def test_hand_built_weights_known_answers(quiet):
    """Rows worked out by hand from the rule (no truncation)."""
    cases = MP.all_cases(quiet)

    def row(name, i):
        with quiet():
            rp, ci, v, _, _ = A.interp_mpass(*cases[name], 0.0)
        return dict(zip(ci[rp[i]:rp[i + 1]].tolist(), v[rp[i]:rp[i + 1]].tolist()))

    # tot = -1 - 0.5 - 0.25, sub = -1 - 0.25, hat w = -1 - 0.25, d = the last diagonal entry 4
    assert row("dup_entries", 0) == {0: -((-1.75 / -1.25) * -1.25) / 4.0}
    assert row("sub_zero", 0) == {0: 0.0, 1: 0.0} and row("d_zero", 0) == {0: 0.0, 1: 0.0}
    assert row("unreached", 0) == {} and row("unreached", 2) == {} and len(row("unreached", 3)) == 1
    assert row("n1_c", 0) == {0: 1.0}
    with quiet():
        assert A.interp_mpass(*cases["chain40"], 0.0)[4] == 39
        assert A.interp_mpass(*cases["all_c"], 0.0)[4] == 0
    # 12 * 12 own C points and the three shared ones, in discovery order
    assert len(row("mstar12", 0)) == 147 and len(row("star130", 0)) == 130 * 130 + 3


@pytest.mark.parametrize("trunc", [MP.TRUNC, 0.0])
@pytest.mark.parametrize("name", CASES)
def test_host_weights_equal_restatement(name, trunc, quiet):
    c = MP.all_cases(quiet)[name]
    with quiet():
        got = A.interp_mpass(c.A, c.S, c.mark, trunc)
    want, passes, unreached = MP.restated(name, c, trunc)
    MP.K.assert_same_p(got[:4], want, (name, trunc))
    assert got[4] == passes
    empty = np.flatnonzero(np.diff(got[0]) == 0)
    assert empty.tolist() == unreached
    if name in MP.STENCILS or name.startswith("p7_24"):
        assert (c.mark[empty] == MP.ISPT).all()   # no F point is unreached


@pytest.mark.parametrize("trunc", [MP.TRUNC, 0.0])
def test_zero_sum_rows_interpolate_constants(trunc, quiet):
    c = MP.all_cases(quiet)["laplacian"]
    with quiet():
        rp, ci, v, _, passes = A.interp_mpass(c.A, c.S, c.mark, trunc)
    rows = np.flatnonzero(np.diff(rp) > 0)
    sums = np.array([np.cumsum(v[rp[i]:rp[i + 1]])[-1] for i in rows])
    print(f"laplacian trunc {trunc}: {len(rows)} rows, {passes} passes, max |sum - 1| = {np.abs(sums - 1.0).max():.3e}")
    assert len(rows) == len(c.mark) and passes >= 2
    assert (np.abs(sums - 1.0) <= 1e-12).all()


_THREADS_CODE = """
import sys, hashlib
sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']
import numpy as np, amg_amd as A, mpass_cases as MP, interp_std_cases as K
from conftest import quiet_ctx
h = hashlib.sha256()
for name in ['p7_24', 'circuit3000']:
    c, _ = MP.coarsened(K.matrix(name), quiet_ctx)
    m1 = A.pmis(*c.S)[0]
    for arr in (*A.agg_graph(*c.S, m1), c.mark, *A.interp_mpass(c.A, c.S, c.mark, 0.2)[:3]):
        h.update(np.ascontiguousarray(arr).tobytes())
print('digest', h.hexdigest())
"""


def test_host_results_do_not_depend_on_the_thread_count():
    """7-pt 24^3 is above the sizes at which the host loops go parallel."""
    out = []
    for threads in ("1", "4"):
        env = dict(os.environ, OMP_NUM_THREADS=threads)
        r = subprocess.run([sys.executable, "-c", _THREADS_CODE, str(ROOT)], env=env, capture_output=True, text=True,
                           check=True)
        out.append([l for l in r.stdout.splitlines() if l.startswith("digest")])
    assert len(out[0]) == 1 and out[0] == out[1]


def test_symbols_exported_declared_and_bound():
    hip = (ROOT / "include" / "sss_hip.h").read_text()
    amg = (ROOT / "include" / "sss_amg.h").read_text()
    for sym in ["sss_agg_graph_host", "sss_hip_agg_graph", "sss_interp_mpass_host", "sss_hip_interp_mpass"]:
        assert sym in A.ABI_SYMBOLS and getattr(A.lib(), sym).argtypes and f"int {sym}(" in hip
    assert "SSS_COARSE_PMIS_AGG = 4" in amg and "intERP_MPASS = 4" in amg
    assert "SSS_COARSE_PMIS = 3" in amg and "intERP_EXTI = 3" in amg
    assert A.COARSE_PMIS_AGG == 4 and A.INTERP_MPASS == 4
    assert callable(A.agg_graph) and callable(A.interp_mpass)


@pytest.mark.skipif(A.device_count() > 0, reason="a GPU is present")
def test_device_functions_fail_without_gpu(quiet):
    c = MP.all_cases(quiet)["repeat_cols"]
    with pytest.raises(RuntimeError) as e:
        A.agg_graph(*c.S, c.mark, device=True)
    assert e.value.rc < 0 and e.value.untouched
    with pytest.raises(RuntimeError) as e:
        A.interp_mpass(c.A, c.S, c.mark, MP.TRUNC, device=True)
    assert e.value.rc < 0 and e.value.untouched


def test_host_error_paths_leave_outputs_untouched(quiet):
    c = MP.all_cases(quiet)["repeat_cols"]
    with pytest.raises(RuntimeError) as e:
        A.agg_graph(*c.S, None)
    assert e.value.rc < 0 and e.value.untouched
    with pytest.raises(RuntimeError) as e:
        A.interp_mpass(c.A, c.S, None, MP.TRUNC)
    assert e.value.rc < 0 and e.value.untouched
    bad = (c.S[0], np.where(c.S[1] == 5, 99, c.S[1]))   # a column out of range
    with pytest.raises(RuntimeError) as e:
        A.interp_mpass(c.A, bad, c.mark, MP.TRUNC)
    assert e.value.rc == -21 and e.value.untouched


# ---------------------------------------------------------------- whole setups
def _shape(H):
    rows = [H.level(l).A.num_rows for l in range(H.num_levels)]
    ops = sum(H.level(l).A.num_nnzs for l in range(H.num_levels)) / H.level(0).A.num_nnzs
    return rows, ops


def _hierarchy(M, quiet, cs=MP.AGG, interp=MP.STD):
    with quiet():
        return A.Hierarchy(M, R.pars(cs, interp))


def test_fewer_rows_and_lower_complexity_than_pmis(quiet):
    M = R.matrix("p7_16")
    H3, H4 = _hierarchy(M, quiet, MP.PMIS), _hierarchy(M, quiet)
    (rows3, ops3), (rows4, ops4) = _shape(H3), _shape(H4)
    print(f"p7_16: cs 3 rows {rows3} ops {ops3:.3f}; cs 4 rows {rows4} ops {ops4:.3f}")
    assert rows4[1] < rows3[1] and ops4 < ops3
    assert int(H4.mg.pars.cs_type) == MP.AGG
    H3.close()
    H4.close()


def test_agg_levels_switch(quiet, monkeypatch):
    M = R.matrix("p7_16")
    H3 = _hierarchy(M, quiet, MP.PMIS)
    H1 = _hierarchy(M, quiet)
    monkeypatch.setenv("SSS_SETUP_AGG_LEVELS", "0")
    H0 = _hierarchy(M, quiet)
    monkeypatch.setenv("SSS_SETUP_AGG_LEVELS", "2")
    H2 = _hierarchy(M, quiet)
    # no aggressive level: the PMIS + interp 2 hierarchy (the digest does not cover pars)
    assert RC.digest(H0) == RC.digest(H3)
    # level 0 is the same with one or two aggressive levels, level 1 is not
    assert RC.same_bits(H1.level(0).P, H2.level(0).P) and RC.same_bits(H1.level(1).A, H2.level(1).A)
    assert H2.num_levels < 3 or not RC.same_bits(H1.level(1).P, H2.level(1).P)
    assert not np.array_equal(RC.cfmark(H1, 1), RC.cfmark(H2, 1))
    for H in (H0, H1, H2, H3):
        H.close()


@pytest.mark.parametrize("cs", [MP.K.RS, MP.PMIS])
def test_multipass_after_the_other_splits(cs, quiet):
    M = R.matrix("p7_16")
    H = _hierarchy(M, quiet, cs, MP.MPASS)
    n = M.num_rows
    assert H.num_levels >= 3
    # level 0 is the multipass P of the split's marks
    c, pinfo = MP.coarsened(M, quiet, cs, MP.MPASS)
    assert pinfo == (n, int((c.mark == MP.CGPT).sum()), False)
    with quiet():
        want = A.interp_mpass(c.A, c.S, c.mark, MP.TRUNC)
    P = H.level(0).P
    MP.K.assert_same_p((*A.csr_arrays(P), P.num_cols), want[:4])
    rtn, rel, _ = oracle_solve(H, np.random.default_rng(1).standard_normal(n), np.zeros(n))
    assert rel[-1] < H.pars.tol and rtn.nits < H.pars.max_it
    H.close()


@pytest.fixture(scope="module")
def agg_16():
    from conftest import quiet_ctx
    with quiet_ctx():
        H = A.Hierarchy(R.matrix("p7_16"), R.pars(MP.AGG, MP.STD))
    yield H
    H.close()


def test_vcycles_converge(agg_16):
    H = agg_16
    n = H.level(0).A.num_rows
    rtn, rel, _ = oracle_solve(H, np.random.default_rng(1).standard_normal(n), np.zeros(n))
    print(f"p7_16 cs 4: {rtn.nits} V-cycles, relres {rel[-1]:.3e}")
    assert rel[-1] < 1e-6 and rtn.nits < H.pars.max_it


def test_hierarchy_file_round_trip(agg_16, tmp_path):
    H = agg_16
    path = tmp_path / "h.sssamg"
    H.save(path)
    G = A.Hierarchy.load(path)
    assert G.num_levels == H.num_levels >= 3
    assert bytes(G.mg.pars) == bytes(H.mg.pars) and G.mg.pars.cs_type == MP.AGG
    assert RC.digest(G) == RC.digest(H)
    for l in range(H.num_levels - 1):
        assert RC.same_bits(G.level(l).P, H.level(l).P) and np.array_equal(RC.cfmark(G, l), RC.cfmark(H, l))
    G.close()


def test_partition_files_take_the_hierarchy(agg_16, tmp_path):
    """sss_part_save on the cs_type 4 hierarchy: every rank's file loads, the replicated tail is the
    hierarchy's levels below the partitioned ones, and the ranks' rows of P on level 0 add up."""
    H = agg_16
    A.part_save(H, 2, tmp_path / "part", 60)
    plans = [A.PartPlan.load(tmp_path / f"part.r{r}") for r in range(2)]
    T = A.Hierarchy.load(tmp_path / "part.tail")
    assert plans[0].nagg >= 1 and T.num_levels == H.num_levels - plans[0].nagg
    for l in range(T.num_levels):
        assert RC.same_bits(T.level(l).A, H.level(plans[0].nagg + l).A)
    assert sum(p.matrix(0, "P").num_nnzs for p in plans) == H.level(0).P.num_nnzs
    assert sum(p.matrix(0, "P").num_rows for p in plans) == H.level(0).P.num_rows
    for p in plans:
        p.close()
    T.close()


@pytest.mark.parametrize("name", ["p7_16", "circuit3000"])
def test_refresh_with_drifted_values_is_a_values_only_recomputation(name, quiet):
    M = RC.matrix(name)
    H = _hierarchy(M, quiet)
    before = [(RC.cfmark(H, l), A.csr_arrays(H.level(l).P)) for l in range(H.num_levels - 1)]
    M2 = RC.drifted(M, 0.3, 0.0)
    H.refresh(M2.mat)
    assert RC.same_bits(H.level(0).A, M2.mat)
    for l in range(H.num_levels - 1):
        L = H.level(l)
        # frozen transfer operators, and the next operator is the Galerkin product of the new values
        assert np.array_equal(RC.cfmark(H, l), before[l][0])
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(A.csr_arrays(L.P), before[l][1]))
        fresh = RC.host_rap(L.R, L.A, L.P)
        assert RC.same_bits(fresh, H.level(l + 1).A)
        A.lib().SSS_mat_destroy(fresh)
    H.close()


def test_refresh_to_a_scaled_operator_is_the_fresh_setup(quiet):
    M = RC.matrix("p7_16")
    M4 = RC.scaled(M, 4.0)
    H = _hierarchy(M, quiet)
    H.refresh(M4.mat)
    F = _hierarchy(M4.mat, quiet)
    assert H.num_levels == F.num_levels and RC.digest(H) == RC.digest(F)
    H.close()
    F.close()


# today's print of the default parameters (the header line ends in a blank)
PRINT_DEFAULT = "\n               AMG Parameters \n" + """\
-----------------------------------------------------------
AMG max num of iter:               100
AMG tol:                           1e-06
AMG ctol:                          1e-07
AMG max levels:                    30
AMG cycle type:                    1
AMG smoother type:                 2
AMG smoother order:                1
AMG num of presmoothing:           2
AMG num of postsmoothing:          2
AMG coarsening type:               {cs}
AMG interPolation type:            {interp}
AMG dof on coarsest grid:          10
AMG strong threshold:              0.3000
AMG truncation threshold:          0.2000
AMG max row sum:                   0.9000
-----------------------------------------------------------
"""


def _pars_in_child(**env_values):
    env = {k: v for k, v in os.environ.items() if k not in ("SSS_SETUP_COARSEN", "SSS_SETUP_INTERP")}
    env.update(env_values)
    code = ("import sys, ctypes as C; sys.path.insert(0, sys.argv[1]); import amg_amd as A; p = A.default_pars(); "
            "print('pars', int(p.cs_type), int(p.interp_type), flush=True); A.lib().SSS_amg_pars_print(C.byref(p)); "
            "C.CDLL(None).fflush(None)")
    r = subprocess.run([sys.executable, "-c", code, str(ROOT)], env=env, capture_output=True, text=True, check=True)
    first, _, rest = r.stdout.partition("\n")
    return first, rest


def test_env_switches_and_parameter_print():
    assert _pars_in_child() == ("pars 1 1", PRINT_DEFAULT.format(cs=1, interp="Dir"))
    assert _pars_in_child(SSS_SETUP_COARSEN="pmis-agg") == ("pars 4 2", PRINT_DEFAULT.format(cs=4, interp="STD"))
    assert _pars_in_child(SSS_SETUP_COARSEN="pmis-agg", SSS_SETUP_INTERP="mpass") == \
        ("pars 4 4", PRINT_DEFAULT.format(cs=4, interp="MPASS"))
    assert _pars_in_child(SSS_SETUP_INTERP="mpass") == ("pars 1 4", PRINT_DEFAULT.format(cs=1, interp="MPASS"))
    assert _pars_in_child(SSS_SETUP_COARSEN="pmis", SSS_SETUP_INTERP="mpass") == \
        ("pars 3 4", PRINT_DEFAULT.format(cs=3, interp="MPASS"))
    assert _pars_in_child(SSS_SETUP_COARSEN="pmis") == ("pars 3 2", PRINT_DEFAULT.format(cs=3, interp="STD"))
    assert _pars_in_child(SSS_SETUP_COARSEN="pmis", SSS_SETUP_INTERP="exti") == \
        ("pars 3 3", PRINT_DEFAULT.format(cs=3, interp="EXTI"))
