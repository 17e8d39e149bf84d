"""CPU: the cap on the entries per row of P (SSS_SETUP_PMAX, sss_interp_trunc_host), an
engine extension that is off by default.  Known answers worked by hand; both host forms (the row-parallel
sss_interp_trunc_host and the in-place serial SSS_amg_interp_trunc, and the latter's route to the
row-parallel form from 2^20 entries) against the plain-Python restatement of the rule
(tests/pmax_cases.py), arrays equal and values bit for bit, on the untruncated P of every standard,
extended+i and multipass case; the invariants of the rule; whole setups with the cap off (today's
hierarchies, by their recorded digests) and on; the hierarchy file, the refresh, the environment switch, the
parameter print and the symbols."""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import amg_amd as A
import interp_std_cases as K
import pmax_cases as PC
import pmis_restatement as R
import refresh_cases as RC
from amg_amd._native import SSS_MAT, iptr
from conftest import oracle_solve

ROOT = Path(__file__).resolve().parent.parent
ERROR_INPUT_PAR = -12   # include/sss_amg.h
DIGESTS = json.loads((ROOT / "tests" / "golden" / "pmax_digests.json").read_text())


@pytest.fixture(autouse=True)
def _cap_off(monkeypatch):
    monkeypatch.delenv("SSS_SETUP_PMAX", raising=False)


def _row(P, i):
    return P[1][P[0][i]:P[0][i + 1]].tolist(), P[2][P[0][i]:P[0][i + 1]].tolist()


# ---------------------------------------------------------------- known answers
def test_known_answers_worked_by_hand():
    """eps 0.0: every entry survives the thresholds."""
    P = PC.hand_p()
    got3 = A.interp_trunc(P[:3], P[3], 0.0, 3)
    got2 = A.interp_trunc(P[:3], P[3], 0.0, 2)
    # six survivors, the three largest are 0.5, 0.3 and -0.4
    ps, ns = 0.5 + 0.3 + 0.05 + 0.2, -0.1 + -0.4
    assert _row(got3, 0) == ([0, 2, 4], [0.5 * (ps / (0.5 + 0.3)), 0.3 * (ps / (0.5 + 0.3)), -0.4 * (ns / -0.4)])
    # |0.5| = |-0.5| are the largest; of |-0.25| = |0.25| the earlier one is third
    ps, ns = 0.5 + 0.25 + 0.125, -0.25 + -0.5
    assert _row(got3, 1) == ([0, 1, 3], [0.5 * (ps / 0.5), -0.25 * (ns / ns), -0.5 * (ns / ns)])
    # the cap of 2 keeps -0.6 and -0.5: the positives are lost and the negatives carry pos_sum + neg_sum
    ps, ns, nk = 0.1 + 0.05, -0.6 + -0.5 + -0.4, -0.6 + -0.5
    cols, vals = _row(got2, 2)
    assert (cols, vals) == ([1, 2], [-0.6 * ((ps + ns) / nk), -0.5 * ((ps + ns) / nk)])
    assert abs(vals[0] + vals[1] - (ps + ns)) <= 4 * np.finfo(float).eps * abs(ps + ns)   # the row sum is unchanged
    # a C row
    assert _row(got3, 3) == ([0], [1.0]) and _row(got2, 3) == ([0], [1.0])
    # and the restatement agrees with the hand
    for got, pmax in [(got3, 3), (got2, 2)]:
        K.assert_same_p(got, PC.restated(P, 0.0, pmax)[0], pmax)


# ---------------------------------------------------------------- host equals restatement; the invariants
def _check_input(itype, name, quiet, monkeypatch):
    P = PC.untruncated(itype, name, quiet)
    longest = int(np.diff(P[0]).max())
    for eps in PC.EPS:
        uncapped = A.interp_trunc(P[:3], P[3], eps, 0)
        K.assert_same_p(uncapped, PC.restated(P, eps, 0)[0], (itype, name, eps))
        monkeypatch.delenv("SSS_SETUP_PMAX", raising=False)
        K.assert_same_p(PC.serial_host_trunc(P, eps), uncapped, (itype, name, eps))
        for pmax in PC.PMAX + [max(longest, 1), longest + 5]:
            what = (itype, name, eps, pmax)
            want, survivors, capped = PC.restated(P, eps, pmax)
            got = A.interp_trunc(P[:3], P[3], eps, pmax)
            K.assert_same_p(got, want, what)
            monkeypatch.setenv("SSS_SETUP_PMAX", str(pmax))
            K.assert_same_p(PC.serial_host_trunc(P, eps), want, what)
            # at most pmax entries per row; rows with at most pmax survivors are the uncapped rows
            assert np.diff(got[0]).max() <= pmax, what
            assert np.array_equal(capped, survivors > pmax)
            for i in np.flatnonzero(~capped):
                assert got[0][i + 1] - got[0][i] == uncapped[0][i + 1] - uncapped[0][i], (what, i)
            keep_g = np.repeat(~capped, np.diff(got[0]))
            keep_u = np.repeat(~capped, np.diff(uncapped[0]))
            assert np.array_equal(got[1][keep_g], uncapped[1][keep_u]), what
            assert np.array_equal(got[2][keep_g].view(np.uint64), uncapped[2][keep_u].view(np.uint64)), what
            if pmax >= longest:   # a no-op
                K.assert_same_p(got, uncapped, what)
    monkeypatch.delenv("SSS_SETUP_PMAX", raising=False)


@pytest.mark.parametrize("itype", [PC.STD, PC.EXTI, PC.MPASS])
def test_host_forms_equal_restatement_and_invariants(itype, quiet, monkeypatch):
    names = [n for t, n in PC.input_names(quiet) if t == itype]
    assert "star130" in names and (itype == PC.MPASS or "star20" in names)
    for name in names:
        _check_input(itype, name, quiet, monkeypatch)


def test_route_to_the_row_parallel_form_above_2_to_20_entries(quiet, monkeypatch):
    """SSS_amg_interp_trunc hands a P of 2^20 entries or more to the row-parallel form: 21 copies of
    star130's rows, among them 21 rows of 16,903 entries."""
    P = PC.untruncated(PC.EXTI, "star130", quiet)
    big = PC.tiled(P, 21)
    assert len(big[1]) >= 1 << 20
    for eps, pmax in [(K.TRUNC, 4), (0.0, 2), (K.TRUNC, 0)]:
        want = PC.tiled(PC.restated(P, eps, pmax)[0], 21)
        monkeypatch.setenv("SSS_SETUP_PMAX", str(pmax))
        K.assert_same_p(PC.serial_host_trunc(big, eps), want, (eps, pmax))


def test_zero_sum_rows_still_interpolate_constants(quiet):
    """p7_12 with both splits, extended+i: the rows of A with zero sum have rows of P with sum 1 whatever
    the cap (1e-12: the tolerance of the uncapped extended+i test)."""
    for tag in ("rs", "pmis"):
        c = K.all_cases(quiet)[f"p7_12_{tag}"]
        arp, _, av = c.A
        asum = np.array([np.cumsum(av[arp[i]:arp[i + 1]])[-1] for i in range(len(c.mark))])
        P = PC.untruncated(PC.EXTI, f"p7_12_{tag}", quiet)
        rows = np.flatnonzero((asum == 0.0) & (np.diff(P[0]) > 0))
        assert len(rows) >= 100
        for eps in PC.EPS:
            for pmax in PC.PMAX:
                rp, _, v, _ = A.interp_trunc(P[:3], P[3], eps, pmax)
                sums = np.array([np.cumsum(v[rp[i]:rp[i + 1]])[-1] for i in rows])
                print(f"p7_12_{tag} eps {eps} pmax {pmax}: {len(rows)} rows, max |sum - 1| = {np.abs(sums - 1.0).max():.3e}")
                assert (np.abs(sums - 1.0) <= 1e-12).all()


_THREADS_CODE = """
import sys, hashlib
sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']
import numpy as np, amg_amd as A, pmax_cases as PC
from conftest import quiet_ctx
h = hashlib.sha256()
for itype, name in [(2, 'p7_24_pmis'), (3, 'p7_24_rs_level1'), (3, 'star130')]:
    P = PC.untruncated(itype, name, quiet_ctx)
    for eps in PC.EPS:
        for pmax in PC.PMAX:
            for arr in A.interp_trunc(P[:3], P[3], eps, pmax)[:3]:
                h.update(np.ascontiguousarray(arr).tobytes())
print('digest', h.hexdigest())
"""


def test_host_result_does_not_depend_on_the_thread_count():
    out = []
    for threads in ("1", "4"):
        env = dict(os.environ, OMP_NUM_THREADS=threads)
        env.pop("SSS_SETUP_PMAX", None)
        r = subprocess.run([sys.executable, "-c", _THREADS_CODE, str(ROOT)], env=env, capture_output=True, text=True,
                           check=True)
        out.append([l for l in r.stdout.splitlines() if l.startswith("digest")])
    assert len(out[0]) == 1 and out[0] == out[1]


# ---------------------------------------------------------------- whole setups
def _hierarchy(M, quiet, cs, interp):
    with quiet():
        return A.Hierarchy(M, R.pars(cs, interp))


def _ops(H):
    return sum(H.level(l).A.num_nnzs for l in range(H.num_levels)) / H.level(0).A.num_nnzs


def _longest_p_row(H):
    return max(int(np.diff(A.csr_arrays(H.level(l).P)[0]).max()) for l in range(H.num_levels - 1))


def _vcycles(H):
    n = H.level(0).A.num_rows
    rtn, rel, _ = oracle_solve(H, np.random.default_rng(1).standard_normal(n), np.zeros(n))
    return rtn.nits, rel[-1]


@pytest.mark.parametrize("cs,interp", PC.HIER)
def test_cap_off_is_todays_hierarchy(cs, interp, quiet, monkeypatch):
    """Unset, 0, not a number, and a cap no row reaches: the hierarchy recorded before the cap existed."""
    M = R.matrix(PC.HIER_MATRIX)
    for value in (None, "0", "-3", "many", "1000"):
        if value is not None:
            monkeypatch.setenv("SSS_SETUP_PMAX", value)
        assert A.setup_pmax() == (1000 if value == "1000" else 0)
        H = _hierarchy(M, quiet, cs, interp)
        assert H.num_levels >= 3 and RC.digest(H) == DIGESTS[PC.hier_key(cs, interp)], (cs, interp, value)
        H.close()


@pytest.mark.parametrize("n", [16, 24])
def test_capped_extended_i_is_cheaper_than_standard_and_no_slower(n, quiet, monkeypatch):
    """PMIS, 7-pt n^3: extended+i with at most 4 entries per row against the uncapped extended+i and the
    uncapped standard interpolation."""
    M = R.matrix(f"p7_{n}")
    H2, H3 = _hierarchy(M, quiet, 3, 2), _hierarchy(M, quiet, 3, 3)
    monkeypatch.setenv("SSS_SETUP_PMAX", "4")
    H3c = _hierarchy(M, quiet, 3, 3)
    monkeypatch.delenv("SSS_SETUP_PMAX")
    (its2, rel2), (its3, rel3), (its3c, rel3c) = _vcycles(H2), _vcycles(H3), _vcycles(H3c)
    print(f"p7_{n} PMIS: interp 2 ops {_ops(H2):.3f} {its2} cycles; interp 3 ops {_ops(H3):.3f} {its3} cycles; "
          f"interp 3 cap 4 ops {_ops(H3c):.3f} {its3c} cycles")
    assert _longest_p_row(H3c) <= 4 < _longest_p_row(H3)
    assert _ops(H3c) < _ops(H2) < _ops(H3)
    assert rel3c < 1e-6 and rel2 < 1e-6 and its3c <= its2 < H2.pars.max_it
    for H in (H2, H3, H3c):
        H.close()


@pytest.mark.parametrize("cs,interp", [(3, 1), (3, 2), (3, 4), (4, 1), (4, 2), (4, 3), (4, 4)])
def test_every_interpolation_takes_the_cap(cs, interp, quiet, monkeypatch, pmax=4):
    monkeypatch.setenv("SSS_SETUP_PMAX", str(pmax))
    H = _hierarchy(R.matrix(PC.HIER_MATRIX), quiet, cs, interp)
    its, rel = _vcycles(H)
    print(f"{PC.HIER_MATRIX} cs {cs} interp {interp} cap {pmax}: ops {_ops(H):.3f}, {its} V-cycles, relres {rel:.3e}")
    assert H.num_levels >= 3 and _longest_p_row(H) <= pmax
    assert rel < H.pars.tol and its < H.pars.max_it
    H.close()


# ---------------------------------------------------------------- plumbing
@pytest.fixture()
def capped_16(quiet, monkeypatch):
    monkeypatch.setenv("SSS_SETUP_PMAX", "4")
    H = _hierarchy(RC.matrix("p7_16"), quiet, 3, 3)
    monkeypatch.delenv("SSS_SETUP_PMAX")
    yield H
    H.close()


def test_hierarchy_file_round_trip(capped_16, tmp_path):
    H = capped_16
    H.save(tmp_path / "h.sssamg")
    G = A.Hierarchy.load(tmp_path / "h.sssamg")
    assert G.num_levels == H.num_levels >= 3 and bytes(G.mg.pars) == bytes(H.mg.pars)
    assert RC.digest(G) == RC.digest(H) and _longest_p_row(G) <= 4
    G.close()


def test_refresh_with_drifted_values_keeps_the_capped_p(capped_16):
    H = capped_16
    M = RC.matrix("p7_16")
    before = [(RC.cfmark(H, l), A.csr_arrays(H.level(l).P)) for l in range(H.num_levels - 1)]
    M2 = RC.drifted(M, 0.3, 0.0)
    H.refresh(M2.mat)
    assert RC.same_bits(H.level(0).A, M2.mat)
    for l in range(H.num_levels - 1):
        L = H.level(l)
        assert np.array_equal(RC.cfmark(H, l), before[l][0])
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(A.csr_arrays(L.P), before[l][1]))
        fresh = RC.host_rap(L.R, L.A, L.P)
        assert RC.same_bits(fresh, H.level(l + 1).A)
        A.lib().SSS_mat_destroy(fresh)
    its, rel = _vcycles(H)
    assert rel < H.pars.tol and its < H.pars.max_it


def _print_in_child(**env_values):
    env = {k: v for k, v in os.environ.items() if k not in ("SSS_SETUP_COARSEN", "SSS_SETUP_INTERP", "SSS_SETUP_PMAX")}
    env.update(env_values)
    code = ("import sys, ctypes as C; sys.path.insert(0, sys.argv[1]); import amg_amd as A; p = A.default_pars(); "
            "print('pmax', A.setup_pmax(), flush=True); A.lib().SSS_amg_pars_print(C.byref(p)); C.CDLL(None).fflush(None)")
    r = subprocess.run([sys.executable, "-c", code, str(ROOT)], env=env, capture_output=True, text=True, check=True)
    first, _, rest = r.stdout.partition("\n")
    return first, rest


def test_env_switch_and_parameter_print():
    from test_agg_mpass import PRINT_DEFAULT
    today = PRINT_DEFAULT.format(cs=1, interp="Dir")
    line = "AMG truncation threshold:          0.2000\n"
    for value in ("0", "-4", "four", ""):
        assert _print_in_child(SSS_SETUP_PMAX=value) == ("pmax 0", today)
    assert _print_in_child() == ("pmax 0", today)
    assert _print_in_child(SSS_SETUP_PMAX="4") == \
        ("pmax 4", today.replace(line, line + "AMG max entries per row of P:      4\n"))


def test_symbols_exported_declared_and_bound():
    hip = (ROOT / "include" / "sss_hip.h").read_text()
    for sym in ["sss_setup_pmax", "sss_interp_trunc_host", "sss_hip_interp_trunc"]:
        assert sym in A.ABI_SYMBOLS and getattr(A.lib(), sym).argtypes is not None and f"int {sym}(" in hip
    assert callable(A.interp_trunc) and callable(A.setup_pmax)
    assert "SSS_SETUP_PMAX" in (ROOT / "include" / "sss_amg.h").read_text()


def _sentinel_p(n=3):
    rp = np.array([0, 2, 3, 4], np.int32)
    ci = np.array([0, 1, 1, 0], np.int32)
    v = np.array([0.5, -7.0, 1.0, 1.0])
    return SSS_MAT(n, 2, 4, iptr(rp), iptr(ci), v.ctypes.data_as(C.POINTER(C.c_double))), (rp, ci, v)


def _untouched(P, keep):
    rp, ci, v = keep
    return (P.num_rows, P.num_cols, P.num_nnzs) == (3, 2, 4) and rp.tolist() == [0, 2, 3, 4] and ci.tolist() == [0, 1, 1, 0] \
        and v.tolist() == [0.5, -7.0, 1.0, 1.0] and C.addressof(P.row_ptr.contents) == rp.ctypes.data \
        and C.addressof(P.col_idx.contents) == ci.ctypes.data and C.addressof(P.val.contents) == v.ctypes.data


@pytest.mark.parametrize("symbol", ["sss_interp_trunc_host", "sss_hip_interp_trunc"])
def test_bad_arguments_are_refused_with_p_untouched(symbol):
    """pmax < 0, a NULL P, row pointers that do not start at 0 or decrease, an entry count that disagrees:
    ERROR_INPUT_PAR from both forms, before anything else happens."""
    fn = getattr(A.lib(), symbol)
    P, keep = _sentinel_p()
    assert fn(C.byref(P), 0.2, -1) == ERROR_INPUT_PAR and _untouched(P, keep)
    assert fn(None, 0.2, 4) == ERROR_INPUT_PAR
    P.num_nnzs = 5
    assert fn(C.byref(P), 0.2, 4) == ERROR_INPUT_PAR
    P.num_nnzs = 4
    for bad in ([1, 2, 3, 4], [0, 3, 2, 4]):
        keep[0][:] = bad
        assert fn(C.byref(P), 0.2, 4) == ERROR_INPUT_PAR
    keep[0][:] = [0, 2, 3, 4]
    P.num_rows = 0
    assert fn(C.byref(P), 0.2, 4) == ERROR_INPUT_PAR
    P.num_rows = 3
    assert _untouched(P, keep)


@pytest.mark.skipif(A.device_count() > 0, reason="a GPU is present")
def test_device_entry_point_fails_without_gpu(quiet):
    P = PC.hand_p()
    for pmax in (0, 3):
        with pytest.raises(RuntimeError) as e:
            A.interp_trunc(P[:3], P[3], 0.2, pmax, device=True)
        assert e.value.rc < 0 and e.value.untouched
