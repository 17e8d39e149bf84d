"""GPU: the extended+i weights on the device (sss_hip_interp_exti, amg_amd/csrc/sss_interp.hip) against the
host's (interp_EXTI): arrays equal and values bit for bit on the hand-built cases, the natural cases with
both splits and the hierarchy levels, with the default truncation and with none, with every lane-group
width, with the per-row tables in LDS and in global memory; whole PMIS + interp 3 setups with the device
path forced build the hierarchy the host path builds; the error paths; the solve phase on a PMIS + ext+i
hierarchy in parity mode (bitwise the oracle) and in throughput mode."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest

import amg_amd as A
import interp_exti_cases as E
import interp_std_cases as K
import pmis_restatement as R
import refresh_cases as RC
from amg_amd._native import SSS_IMAT, SSS_MAT, NumpyCSR, iptr
from conftest import oracle_solve, quiet_ctx

pytestmark = pytest.mark.gpu

EXTI = 3
ERROR_DATA_STRUCTURE = -21
NATURAL = [f"{n}_{t}" for t in ["rs", "pmis"] for n in K.NATURAL]
_host = {}


def host_weights(name, c, trunc):
    """The host result of a case, computed once."""
    if (name, trunc) not in _host:
        with quiet_ctx():
            _host[name, trunc] = A.interp_exti(c.A, c.S, c.mark, c.P, trunc)
    return _host[name, trunc]


def check_weights(name, c, trunc):
    got = A.interp_exti(c.A, c.S, c.mark, c.P, trunc, device=True)
    K.assert_same_p(got, host_weights(name, c, trunc), (name, trunc))


@pytest.mark.parametrize("trunc", [K.TRUNC, 0.0])
@pytest.mark.parametrize("name", NATURAL + E.HAND)
def test_device_weights_equal_host(name, trunc, quiet):
    check_weights(name, E.all_cases(quiet)[name], trunc)


@pytest.mark.parametrize("trunc", [K.TRUNC, 0.0])
def test_device_weights_on_hierarchy_levels(trunc, quiet):
    cases = E.all_cases(quiet)
    names = [k for k in cases if "_level" in k]
    assert len(names) >= 8
    for name in names:
        check_weights(name, cases[name], trunc)


@pytest.mark.parametrize("lanes", ["1", "4", "16", "64"])
def test_every_lane_group_width(lanes, quiet, monkeypatch):
    """Each width walks short rows, the longest natural rows, a coarse PMIS level, a 403-entry pattern
    row whose neighbours' rows span several chunks, and the small cases, whatever their average."""
    monkeypatch.setenv("SSS_HIP_INTERP_LANES", lanes)
    cases = E.all_cases(quiet)
    for name in ["a27_8_rs", "p7_24_rs_level3", "circuit3000_pmis_level2", "star20"] + E.SMALL:
        for trunc in [K.TRUNC, 0.0]:
            check_weights(name, cases[name], trunc)


def global_rows(err):
    m = re.findall(r"extended\+i P: device weights,.* (\d+) rows on global tables", err)
    assert len(m) == 1, err
    return int(m[0])


@pytest.mark.parametrize("name,slots", [("star130", None), ("star130", "64"), ("star20", "64"), ("p7_24_rs_level2", "64")])
def test_global_table_path(name, slots, quiet, monkeypatch, capfd):
    """Rows whose candidate bound exceeds the LDS table take a table in global memory inside the same
    call: star(130)'s 16903-entry row with nothing forced, the others with the LDS table lowered."""
    monkeypatch.setenv("SSS_SETUP_TIMING", "1")
    if slots:
        monkeypatch.setenv("SSS_HIP_INTERP_LDS_SLOTS", slots)
    c = E.all_cases(quiet)[name]
    host = [host_weights(name, c, t) for t in [K.TRUNC, 0.0]]
    capfd.readouterr()
    for trunc, want in zip([K.TRUNC, 0.0], host):
        check_weights(name, c, trunc)
        assert global_rows(capfd.readouterr().err) > 0


@pytest.mark.parametrize("case", ["p7_24", "circuit3000"])
def test_setup_with_device_interpolation_same_hierarchy(case, monkeypatch, capfd):
    M = R.matrix(case)
    monkeypatch.setenv("SSS_SETUP_TIMING", "1")
    monkeypatch.setenv("SSS_SETUP_GPU_INTERP", "0")
    with quiet_ctx():
        H = A.Hierarchy(M, R.pars(R.PMIS, EXTI))
    d_host, levels = RC.digest(H), H.num_levels
    H.close()
    err = capfd.readouterr().err
    # one pattern and one weight computation per coarsened level (the level loop may discard the last)
    assert err.count("standard P: host pattern") >= levels - 1 and err.count("extended+i P: host weights") >= levels - 1
    assert "device pattern" not in err and "device weights" not in err
    monkeypatch.setenv("SSS_SETUP_GPU_INTERP", "1")
    monkeypatch.setenv("SSS_SETUP_GPU_INTERP_MIN", "0")
    with quiet_ctx():
        H = A.Hierarchy(M, R.pars(R.PMIS, EXTI))
    d_dev = RC.digest(H)
    H.close()
    err = capfd.readouterr().err
    assert err.count("standard P: device pattern") >= levels - 1 and err.count("extended+i P: device weights") >= levels - 1
    assert "host pattern" not in err and "host weights" not in err
    assert levels >= 3 and d_dev == d_host


def _sentinel_p(n):
    rp = np.zeros(n + 1, np.int32)
    ci = np.full(4, -7, np.int32)
    v = np.full(4, -7.0)
    return SSS_MAT(n, -7, 0, iptr(rp), iptr(ci), v.ctypes.data_as(C.POINTER(C.c_double))), (rp, ci, v)


def _untouched(P, keep, n):
    rp, ci, v = keep
    return (P.num_rows, P.num_cols, P.num_nnzs) == (n, -7, 0) and (rp == 0).all() and (ci == -7).all() and (v == -7.0).all() \
        and C.addressof(P.row_ptr.contents) == rp.ctypes.data and C.addressof(P.col_idx.contents) == ci.ctypes.data \
        and C.addressof(P.val.contents) == v.ctypes.data


def test_error_paths_nothing_launched(quiet):
    """Zero rows, and a NULL mark: an error code, P's fields untouched (the checks precede every HIP call)."""
    c = E.all_cases(quiet)["plus_i"]
    n = len(c.mark)
    Am = NumpyCSR(*c.A)
    for rows, mark in [(0, iptr(c.mark)), (n, None)]:
        S = SSS_IMAT(rows, rows, len(c.S[1]), iptr(c.S[0]), iptr(c.S[1]), None)
        P, keep = _sentinel_p(n)
        assert A.lib().sss_hip_interp_exti(C.byref(Am.mat), C.byref(S), mark, C.byref(P), K.TRUNC) < 0
        assert _untouched(P, keep, n)


def test_inconsistent_s_is_an_error_code(capfd):
    """Row 0 of S names a column row 0 of A does not have.  The kernel treats it as data: the search of
    the row finds nothing, the flag is raised, and the call fails with P untouched."""
    c = K.inconsistent_case()
    n = len(c.mark)
    Am = NumpyCSR(*c.A)
    S = SSS_IMAT(n, n, len(c.S[1]), iptr(c.S[0]), iptr(c.S[1]), None)
    lib = A.lib()
    P = lib.SSS_mat_struct_create(n, int((c.mark == K.CGPT).sum()), len(c.P[1]))
    C.memmove(P.row_ptr, c.P[0].ctypes.data, c.P[0].nbytes)
    C.memmove(P.col_idx, c.P[1].ctypes.data, c.P[1].nbytes)
    sentinel = np.full(len(c.P[1]), -7.0)
    C.memmove(P.val, sentinel.ctypes.data, sentinel.nbytes)

    def fields():
        return (P.num_rows, P.num_cols, P.num_nnzs, C.addressof(P.row_ptr.contents), C.addressof(P.col_idx.contents),
                C.addressof(P.val.contents))

    before = fields()
    rc = lib.sss_hip_interp_exti(C.byref(Am.mat), C.byref(S), iptr(c.mark), C.byref(P), K.TRUNC)
    assert rc == ERROR_DATA_STRUCTURE
    assert "strong column absent" in capfd.readouterr().err
    assert fields() == before
    rp, ci, v = A.csr_arrays(P)
    assert np.array_equal(rp, c.P[0]) and np.array_equal(ci, c.P[1]) and (v == -7.0).all()
    lib.SSS_mat_destroy(C.byref(P))
    with pytest.raises(RuntimeError) as e:
        A.interp_exti(c.A, c.S, c.mark, c.P, K.TRUNC, device=True)
    assert e.value.rc == rc


@pytest.fixture(scope="module")
def exti_16():
    with quiet_ctx():
        H = A.Hierarchy(R.matrix("p7_16"), R.pars(R.PMIS, EXTI))
    yield H
    H.close()


def test_parity_mode_solve_is_the_oracles(exti_16):
    H = exti_16
    n = H.level(0).A.num_rows
    b = np.random.default_rng(1).standard_normal(n)
    rtn, rel_r, _ = oracle_solve(H, b, x_r := np.zeros(n))
    assert rel_r[-1] < H.pars.tol
    D = A.DeviceHierarchy(H, smoother="exact", coarse="krylov")
    try:
        D.upload(0, "b", b)
        D.upload(0, "x", np.zeros(n))
        rel_g = []
        while len(rel_g) < 100:   # the solve loop: cycle until the relative residual is below tol
            D.cycle()
            rel_g.append(D.residual_norm() / np.sqrt(np.dot(b, b)))
            if rel_g[-1] < H.pars.tol:
                break
        x_g = D.download(0, "x")
    finally:
        D.close()
    assert len(rel_g) == rtn.nits
    assert np.array_equal(x_g.view(np.uint64), x_r.view(np.uint64))


def test_throughput_mode_pcg_converges(exti_16):
    H = exti_16
    n = H.level(0).A.num_rows
    D = A.DeviceHierarchy(H, smoother="hybrid", coarse="direct")
    try:
        D.upload(0, "b", np.random.default_rng(1).standard_normal(n))
        D.upload(0, "x", np.zeros(n))
        its, hist = D.pcg(1e-6, 100)
    finally:
        D.close()
    print(f"p7_16 PMIS + ext+i: pcg {its} iterations, {hist[-1]:.3e}")
    assert hist[-1] < 1e-6 and its < 100
