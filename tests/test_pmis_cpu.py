"""PMIS coarsening (cs_type 3, an engine extension), host side: the OpenMP split of
amg_amd/host/sss_setup.c against the numpy restatement of the rule (tests/pmis_restatement.py), its
invariants, its independence of the thread count, the hash's known answers, the hierarchies it builds
with interp_type 2 (level sizes, convergence of the oracle's solve, iterations against RS), the
SSS_SETUP_COARSEN switch and the interp_type 1 combination."""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import amg_amd as A
import pmis_restatement as R
from conftest import oracle_solve

ROOT = Path(__file__).resolve().parent.parent

S_NAMES = ["p7_12", "p7_24", "a27_8", "circuit3000", "bus", "n1", "empty_row", "lambda0_neighbour",
           "nobody_depends", "long_row_700", "n257", "n1025", "n4097_long"]


def test_hash_known_answers():
    assert [int(v) for v in R.h32([0, 1, 2, 12345])] == [0, 0x688990C0, 0xD1132181, 0x912EFCF7]
    # a bijection on a window: no two of 2^16 consecutive arguments collide
    assert len(np.unique(R.h32(np.arange(1 << 16)))) == 1 << 16


@pytest.mark.parametrize("name", S_NAMES)
def test_host_split_equals_restatement(name, quiet):
    rp, ci = R.all_s(quiet)[name]
    want, nc_want, rounds_want = R.pmis_restated(rp, ci)
    mark, nc, rounds = A.pmis(rp, ci)
    assert np.array_equal(mark, want)
    assert (nc, rounds) == (nc_want, rounds_want)
    # the stencils' S has a symmetric pattern: there no two C points are neighbours in either direction
    R.check_invariants(rp, ci, mark, nc, symmetric=True if name in ("p7_12", "p7_24") else None)


def test_host_split_on_hierarchy_levels(quiet):
    """Every level of the PMIS hierarchies of 7-pt 24^3 and the circuit: the coarse levels' S rows are
    longer than the lane group the device split gives them (16; hand-built long_row_700 has the rest)."""
    names = [k for k in R.all_s(quiet) if "_level" in k]
    assert sum(k.startswith("p7_24") for k in names) >= 3 and sum(k.startswith("circuit") for k in names) >= 3
    longest = 0
    for name in names:
        rp, ci = R.all_s(quiet)[name]
        longest = max(longest, int(np.diff(rp).max()))
        want, nc_want, rounds_want = R.pmis_restated(rp, ci)
        mark, nc, rounds = A.pmis(rp, ci)
        assert np.array_equal(mark, want), name
        assert (nc, rounds) == (nc_want, rounds_want), name
        R.check_invariants(rp, ci, mark, nc)
    assert longest > 16


def test_coarsen_returns_the_split(quiet):
    """SSS_amg_coarsen with cs_type 3 hands back the restatement's marks."""
    for name in ["p7_12", "bus"]:
        M = R.matrix(name)
        (rp, ci), mark, rc = R.strength(M, quiet)
        want, nc, _ = R.pmis_restated(rp, ci)
        assert rc == 0 and np.array_equal(mark, want)


_CHILD = r"""
import hashlib, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import amg_amd as A
import pmis_restatement as R
from conftest import quiet_ctx
h = hashlib.sha256()
for name in ["p7_24", "a27_8", "circuit3000"]:
    (rp, ci), _, rc = R.strength(R.matrix(name), quiet_ctx)
    mark, nc, rounds = A.pmis(rp, ci)
    h.update(mark.tobytes()); h.update(bytes([rounds])); h.update(nc.to_bytes(4, "little"))
rp, ci = R.random_s(20001, 11, maxrow=12)
mark, nc, rounds = A.pmis(rp, ci)
h.update(mark.tobytes())
print("digest", h.hexdigest())
"""


def test_marks_do_not_depend_on_the_thread_count():
    out = {}
    for t in ("1", "8"):
        env = dict(os.environ, OMP_NUM_THREADS=t)
        r = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT)], env=env, capture_output=True, text=True, check=True)
        out[t] = [l for l in r.stdout.splitlines() if l.startswith("digest")]
        assert len(out[t]) == 1, r.stdout + r.stderr
    assert out["1"] == out["8"]


# rows per level of the PMIS + interp_type 2 hierarchies (DESIGN.md "PMIS coarsening")
LEVEL_ROWS = {
    "p7_12": [1728, 594, 85],
    "p7_16": [4096, 1358, 186, 34],
    "a27_8": [512, 102],
    "bus": [1138, 398, 119, 30],
    "circuit3000": [3000, 1150, 339, 79],
}


@pytest.mark.parametrize("name", list(LEVEL_ROWS))
def test_pmis_hierarchy(name, quiet):
    M = R.matrix(name)
    n = M.num_rows
    with quiet():
        H = A.Hierarchy(M, R.pars(R.PMIS, R.STD))
        Hrs = A.Hierarchy(M, R.pars(A.COARSE_RS, R.STD))
    rows = [H.level(l).A.num_rows for l in range(H.num_levels)]
    for l in range(H.num_levels - 1):
        L = H.level(l)
        assert (L.P.num_rows, L.P.num_cols) == (rows[l], rows[l + 1])
        assert (L.R.num_rows, L.R.num_cols) == (rows[l + 1], rows[l])
        cf = np.ctypeslib.as_array(L.cfmark.d, shape=(rows[l],))
        assert int((cf == R.CGPT).sum()) == rows[l + 1]
    b = np.random.default_rng(1).standard_normal(n)
    rtn, rel, _ = oracle_solve(H, b, np.zeros(n))
    rtn_rs, rel_rs, _ = oracle_solve(Hrs, b, np.zeros(n))
    print(f"{name}: PMIS rows {rows} its {rtn.nits} relres {rel[-1]:.3e}; RS its {rtn_rs.nits}")
    assert rel[-1] < H.pars.tol and rtn.nits < 100
    assert rel_rs[-1] < Hrs.pars.tol
    assert rows == LEVEL_ROWS[name]
    assert rtn.nits <= 2 * rtn_rs.nits + 2
    H.close()
    Hrs.close()


def _pars_in_child(env_value):
    env = {k: v for k, v in os.environ.items() if k != "SSS_SETUP_COARSEN"}
    if env_value is not None:
        env["SSS_SETUP_COARSEN"] = env_value
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import amg_amd as A; p = A.default_pars(); "
            "print('pars', int(p.cs_type), int(p.interp_type))")
    r = subprocess.run([sys.executable, "-c", code, str(ROOT)], env=env, capture_output=True, text=True, check=True)
    return [l for l in r.stdout.splitlines() if l.startswith("pars")]


def test_env_switch_in_pars_init():
    assert _pars_in_child("pmis") == ["pars 3 2"]
    assert _pars_in_child(None) == ["pars 1 1"]
    assert _pars_in_child("rs") == ["pars 1 1"]
    assert A.COARSE_PMIS == 3


def test_pmis_with_direct_interpolation_builds_and_runs(quiet):
    """cs_type 3 with interp_type 1: allowed, the F-F cleanup is skipped (the weak combination);
    only the shape is asserted."""
    M = R.matrix("p7_12")
    n = M.num_rows
    with quiet():
        H = A.Hierarchy(M, R.pars(R.PMIS, 1))
    assert H.num_levels >= 2
    (rp, ci), _, _ = R.strength(M, quiet)
    want, nc, _ = R.pmis_restated(rp, ci)
    cf = np.ctypeslib.as_array(H.level(0).cfmark.d, shape=(n,))
    assert np.array_equal(cf, want)   # no cleanup touched the marks
    for l in range(H.num_levels - 1):
        L = H.level(l)
        assert L.P.num_rows == L.A.num_rows and L.P.num_cols == H.level(l + 1).A.num_rows
    rtn, rel, _ = oracle_solve(H, np.ones(n), np.zeros(n))
    assert rtn.nits >= 1 and np.isfinite(rel).all()
    H.close()
