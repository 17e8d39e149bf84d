"""CPU: the extended+i interpolation (interp_type 3, an engine extension), host side.
The OpenMP weights of amg_amd/host/sss_setup.c (interp_EXTI) are bitwise the plain-Python restatement of
the rule (tests/interp_exti_cases.py) on the hand-built and the natural cases with both splits and both
truncations; rows of A with zero sum get rows of P with sum 1; the PMIS + interp 3 hierarchy builds,
converges in no more iterations than PMIS + interp 2 and in fewer at 24^3 and 32^3; the new symbol, the
SSS_SETUP_INTERP switch and the parameter print; the hierarchy file and the refresh."""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import amg_amd as A
import interp_exti_cases as E
import interp_std_cases as K
import pmis_restatement as R
import refresh_cases as RC
from conftest import oracle_solve

ROOT = Path(__file__).resolve().parent.parent
EXTI = 3
CASES = E.HAND + [f"{n}_{t}" for n in E.NATURAL for t in ("rs", "pmis")]


def test_hand_cases_known_answers(quiet):
    """Row 0 of the hand-built cases, worked out by hand from the rule (no truncation)."""
    cases = E.all_cases(quiet)

    def row0(name):
        (rp, ci, v, _), _ = E.restated(name, cases[name], 0.0)
        return dict(zip(ci[rp[0]:rp[1]].tolist(), v[rp[0]:rp[1]].tolist()))

    # both a_01 and a_02 go to d: d = 5 - 1 - 1.5, ahat[3] = -2
    assert row0("den_zero") == {0: 2.0 / 2.5}
    # den = -2, f = 0.625: d = 4 - 0.625, ahat[2] = -0.625 - 1.5, ahat[3] untouched
    got = row0("same_sign_skipped")
    assert got[0] == 2.125 / 3.375 and got[1] == 0.0
    # den = -3.5, f = -2 / -3.5: ahat[2] = -1.5 f, ahat[3] = -0.125 - f, d = 4 - f - 0.0625
    f = -2.0 / -3.5
    got = row0("weak_in_pattern")
    assert got == {0: -(f * -1.5) / (4.0 + f * -1.0 + -0.0625), 1: -(-0.125 + f * -1.0) / (4.0 + f * -1.0 + -0.0625)}
    # den = -2.25, f = 1 / 2.25: d = 3 - 0.75 f, ahat[2] = -1.5 f - 1
    f = -1.0 / -2.25
    assert row0("plus_i") == {0: -(f * -1.5 + -1.0) / (3.0 + f * -0.75)}
    # den = -1.5: all of a_01 arrives at ahat[2]; the row of A sums to 1, d = 3
    f = -1.0 / -1.5
    assert row0("nonsym_no_aki") == {0: -(f * -1.5 + -1.0) / 3.0}


@pytest.mark.parametrize("trunc", [K.TRUNC, 0.0])
@pytest.mark.parametrize("name", CASES)
def test_host_weights_equal_restatement(name, trunc, quiet):
    c = E.all_cases(quiet)[name]
    with quiet():
        got = A.interp_exti(c.A, c.S, c.mark, c.P, trunc)
    want, _ = E.restated(name, c, trunc)
    K.assert_same_p(got, want, (name, trunc))
    assert np.isfinite(got[2]).all()
    if trunc == 0.0:
        assert np.array_equal(got[0], c.P[0])   # nothing dropped


@pytest.mark.parametrize("trunc", [K.TRUNC, 0.0])
@pytest.mark.parametrize("tag", ["rs", "pmis"])
def test_zero_sum_rows_interpolate_constants(tag, trunc, quiet):
    name = f"p7_12_{tag}"
    c = E.all_cases(quiet)[name]
    with quiet():
        rp, ci, v, _ = A.interp_exti(c.A, c.S, c.mark, c.P, trunc)
    _, rows = E.restated(name, c, trunc)
    assert len(rows) >= 100
    sums = np.array([np.cumsum(v[rp[i]:rp[i + 1]])[-1] for i in rows])
    print(f"{name} trunc {trunc}: {len(rows)} rows, max |sum - 1| = {np.abs(sums - 1.0).max():.3e}")
    assert (np.abs(sums - 1.0) <= 1e-12).all()


def test_symbol_exported_declared_and_bound():
    header = (ROOT / "include" / "sss_hip.h").read_text()
    assert "sss_hip_interp_exti" in A.ABI_SYMBOLS
    assert A.lib().sss_hip_interp_exti.argtypes
    assert "int sss_hip_interp_exti(" in header
    assert "intERP_EXTI = 3" in (ROOT / "include" / "sss_amg.h").read_text()
    assert callable(A.interp_exti)


@pytest.mark.skipif(A.device_count() > 0, reason="a GPU is present")
def test_device_function_fails_without_gpu(quiet):
    c = E.all_cases(quiet)["plus_i"]
    with pytest.raises(RuntimeError) as e:
        A.interp_exti(c.A, c.S, c.mark, c.P, K.TRUNC, device=True)
    assert e.value.rc < 0


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


def test_env_switch_and_parameter_print():
    assert _pars_in_child() == ("pars 1 1", PRINT_DEFAULT.format(cs=1, interp="Dir"))
    assert _pars_in_child(SSS_SETUP_COARSEN="pmis") == ("pars 3 2", PRINT_DEFAULT.format(cs=3, interp="STD"))
    assert _pars_in_child(SSS_SETUP_COARSEN="pmis", SSS_SETUP_INTERP="exti") == \
        ("pars 3 3", PRINT_DEFAULT.format(cs=3, interp="EXTI"))
    assert _pars_in_child(SSS_SETUP_INTERP="exti") == ("pars 1 3", PRINT_DEFAULT.format(cs=1, interp="EXTI"))
    assert _pars_in_child(SSS_SETUP_INTERP="std") == ("pars 1 1", PRINT_DEFAULT.format(cs=1, interp="Dir"))


def _solve(M, interp):
    n = M.num_rows
    H = A.Hierarchy(M, R.pars(R.PMIS, interp))
    rows = [H.level(l).A.num_rows for l in range(H.num_levels)]
    ops = sum(H.level(l).A.num_nnzs for l in range(H.num_levels)) / H.level(0).A.num_nnzs
    rtn, rel, _ = oracle_solve(H, np.random.default_rng(1).standard_normal(n), np.zeros(n))
    tol = H.pars.tol
    H.close()
    return rows, ops, rtn.nits, rel[-1], tol


@pytest.mark.parametrize("name,fewer", [("p7_12", False), ("p7_16", False), ("p7_24", True), ("p7_32", True),
                                        ("a27_8", False), ("bus", False), ("circuit3000", False)])
def test_pmis_exti_hierarchy_converges_no_slower_than_std(name, fewer, quiet):
    """The setup builds with cs_type 3 and interp_type 3 (it exits with ERROR_AMG_interp_type without
    the feature); the oracle's solve converges in no more iterations than on PMIS + interp 2, and in
    strictly fewer on 7-pt 24^3 and 32^3."""
    M = R.matrix(name)
    with quiet():
        rows_s, ops_s, its_s, rel_s, tol = _solve(M, R.STD)
        rows_e, ops_e, its_e, rel_e, _ = _solve(M, EXTI)
    print(f"{name}: std rows {rows_s} ops {ops_s:.2f} its {its_s}; ext+i rows {rows_e} ops {ops_e:.2f} its {its_e}")
    assert rel_s < tol and rel_e < tol and its_e < 100
    assert its_e <= its_s
    if fewer:
        assert its_e < its_s


def _exti_hierarchy(M, quiet):
    with quiet():
        return A.Hierarchy(M, R.pars(R.PMIS, EXTI))


def test_hierarchy_file_round_trip(tmp_path, quiet):
    H = _exti_hierarchy(R.matrix("p7_16"), quiet)
    assert H.num_levels >= 3
    path = tmp_path / "h.sssamg"
    H.save(path)
    G = A.Hierarchy.load(path)
    assert G.num_levels == H.num_levels
    assert bytes(G.mg.pars) == bytes(H.mg.pars) and G.mg.pars.interp_type == EXTI
    assert RC.digest(G) == RC.digest(H)
    for l in range(H.num_levels):
        assert RC.same_bits(G.level(l).A, H.level(l).A)
        if l + 1 < H.num_levels:
            assert RC.same_bits(G.level(l).P, H.level(l).P) and RC.same_bits(G.level(l).R, H.level(l).R)
            assert np.array_equal(RC.cfmark(G, l), RC.cfmark(H, l))
    G.close()
    H.close()


@pytest.mark.parametrize("name", ["p7_16", "circuit3000"])
def test_refresh_to_a_scaled_operator_is_the_fresh_setup(name, quiet):
    M = RC.matrix(name)
    M4 = RC.scaled(M, 4.0)
    H = _exti_hierarchy(M, quiet)
    H.refresh(M4.mat)
    F = _exti_hierarchy(M4.mat, quiet)
    assert H.num_levels == F.num_levels
    assert RC.digest(H) == RC.digest(F)
    H.close()
    F.close()
