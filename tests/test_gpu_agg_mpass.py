"""GPU: the device twins of aggressive coarsening and multipass interpolation (sss_hip_agg_graph,
sss_hip_interp_mpass, amg_amd/csrc/sss_interp.hip) against the host's: S2 and P arrays equal
and values bit for bit on the hand-built cases, the natural cases and the hierarchy levels, with the default
truncation and with none, with every lane-group width, with the per-row tables in LDS and in global memory;
whole cs_type 4 setups with the device path forced build the hierarchy the host path builds; the error paths;
the solve phase on a cs_type 4 hierarchy in parity mode (bitwise the oracle) and in throughput mode; the
mirror's refresh."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest

import amg_amd as A
import interp_std_cases as K
import mpass_cases as MP
import pmis_restatement as R
import refresh_cases as RC
from amg_amd._native import SSS_HIP_LEVEL_INFO, SSS_IMAT, SSS_MAT, NumpyCSR, iptr
from conftest import oracle_solve, quiet_ctx

pytestmark = pytest.mark.gpu

ERROR_DATA_STRUCTURE = -21
LEVELS = [f"p7_24_level{l}" for l in range(3)]
_host = {}


def host_graph(name, c):
    if name not in _host:
        with quiet_ctx():
            m1 = A.pmis(*c.S)[0]
            _host[name] = (m1, A.agg_graph(*c.S, m1))
    return _host[name]


def host_p(name, c, trunc):
    if (name, trunc) not in _host:
        with quiet_ctx():
            _host[name, trunc] = A.interp_mpass(c.A, c.S, c.mark, trunc)
    return _host[name, trunc]


def check_graph(name, c):
    m1, want = host_graph(name, c)
    MP.assert_same_graph(A.agg_graph(*c.S, m1, device=True), want, name)
    # and on the final marks, which select other rows
    with quiet_ctx():
        want = A.agg_graph(*c.S, c.mark)
    MP.assert_same_graph(A.agg_graph(*c.S, c.mark, device=True), want, name)


def check_p(name, c, trunc):
    got, want = A.interp_mpass(c.A, c.S, c.mark, trunc, device=True), host_p(name, c, trunc)
    K.assert_same_p(got[:4], want[:4], (name, trunc))
    assert got[4] == want[4]


@pytest.mark.parametrize("name", MP.NATURAL + LEVELS + MP.HAND)
def test_device_graph_equals_host(name, quiet):
    check_graph(name, MP.all_cases(quiet)[name])


@pytest.mark.parametrize("trunc", [MP.TRUNC, 0.0])
@pytest.mark.parametrize("name", MP.NATURAL + LEVELS + MP.HAND)
def test_device_p_equals_host(name, trunc, quiet):
    check_p(name, MP.all_cases(quiet)[name], trunc)


@pytest.mark.parametrize("lanes", ["1", "4", "16", "64"])
def test_every_lane_group_width(lanes, quiet, monkeypatch):
    """Each width walks short rows, the longest natural rows, a coarse level, the 180-candidate row whose
    neighbours' rows span several chunks, and the small cases, whatever their average."""
    monkeypatch.setenv("SSS_HIP_INTERP_LANES", lanes)
    cases = MP.all_cases(quiet)
    for name in ["a27_8", "p7_12", "circuit3000", "p7_24_level1", "mstar12"] + MP.SMALL:
        check_graph(name, cases[name])
        for trunc in [MP.TRUNC, 0.0]:
            check_p(name, cases[name], trunc)


def global_rows(err, what):
    m = re.findall(what + r": device,.* (\d+) rows on global tables", err)
    assert len(m) == 1, err
    return int(m[0])


@pytest.mark.parametrize("name,slots", [("star130", None), ("mstar12", "64"), ("p7_24_level2", "64")])
def test_global_table_path(name, slots, quiet, monkeypatch, capfd):
    """Rows whose candidate bound exceeds the group's LDS table take a table in global memory inside the
    same call.  P: star130's 17290-candidate row with nothing forced (a group of 64 lanes has 512 slots),
    the 180-candidate row of mstar12 against 64 slots, a row of 9 candidates in a pass of one lane per row
    (8 slots) on the 7-pt 24^3 level.  S2: the stage-one C point of the stars that reaches every other one
    (17550 and 204 candidates at one lane per row), 26 rows of more than 64 candidates on the level."""
    monkeypatch.setenv("SSS_SETUP_TIMING", "1")
    if slots:
        monkeypatch.setenv("SSS_HIP_INTERP_LDS_SLOTS", slots)
    c = MP.all_cases(quiet)[name]
    for trunc in [MP.TRUNC, 0.0]:
        host_p(name, c, trunc)
    m1, want = host_graph(name, c)
    capfd.readouterr()
    for trunc in [MP.TRUNC, 0.0]:
        check_p(name, c, trunc)
        assert global_rows(capfd.readouterr().err, "multipass P") > 0
    MP.assert_same_graph(A.agg_graph(*c.S, m1, device=True), want, name)
    assert global_rows(capfd.readouterr().err, "aggressive S2") > 0


@pytest.mark.parametrize("case", ["p7_24", "circuit3000"])
def test_setup_on_the_device_same_hierarchy(case, monkeypatch, capfd):
    M = R.matrix(case)
    monkeypatch.setenv("SSS_SETUP_TIMING", "1")
    for v in ("SSS_SETUP_GPU_AGG", "SSS_SETUP_GPU_INTERP", "SSS_SETUP_GPU_PMIS"):
        monkeypatch.setenv(v, "0")
    with quiet_ctx():
        H = A.Hierarchy(M, R.pars(MP.AGG, MP.STD))
    d_host, levels = RC.digest(H), H.num_levels
    H.close()
    err = capfd.readouterr().err
    assert err.count("aggressive S2: host") == 1 and err.count("aggressive stage-two split: host") == 1
    assert err.count("multipass P: host") == 1 and "device" not in err
    for v in ("SSS_SETUP_GPU_AGG", "SSS_SETUP_GPU_INTERP", "SSS_SETUP_GPU_PMIS"):
        monkeypatch.setenv(v, "1")
        monkeypatch.setenv(v + "_MIN", "0")
    with quiet_ctx():
        H = A.Hierarchy(M, R.pars(MP.AGG, MP.STD))
    d_dev = RC.digest(H)
    H.close()
    err = capfd.readouterr().err
    assert err.count("aggressive S2: device") == 1 and err.count("aggressive stage-two split: device") == 1
    assert err.count("multipass P: device") == 1
    assert "aggressive S2: host" not in err and "multipass P: host" not in err and "host split" not in err
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


def _sentinel_s2():
    rp = np.full(2, -7, np.int32)
    return SSS_IMAT(-7, -7, -7, iptr(rp), None, None), rp


def _untouched_s2(S2, rp):
    return (S2.num_rows, S2.num_cols, S2.num_nnzs) == (-7, -7, -7) and (rp == -7).all() and not S2.col_idx \
        and C.addressof(S2.row_ptr.contents) == rp.ctypes.data


def test_error_paths_nothing_launched(quiet):
    """Zero rows, and a NULL mark: an error code, the outputs' fields untouched (the checks precede every HIP call)."""
    c = MP.all_cases(quiet)["repeat_cols"]
    n = len(c.mark)
    Am = NumpyCSR(*c.A)
    passes = C.c_int(-7)
    for rows, mark in [(0, iptr(c.mark)), (n, None)]:
        S = SSS_IMAT(rows, rows, len(c.S[1]), iptr(c.S[0]), iptr(c.S[1]), None)
        P, keep = _sentinel_p(n)
        assert A.lib().sss_hip_interp_mpass(C.byref(Am.mat), C.byref(S), mark, C.byref(P), MP.TRUNC, C.byref(passes)) < 0
        assert _untouched(P, keep, n) and passes.value == -7
        S2, rp = _sentinel_s2()
        assert A.lib().sss_hip_agg_graph(C.byref(S), mark, C.byref(S2)) < 0
        assert _untouched_s2(S2, rp)


def test_inconsistent_s_is_an_error_code(capfd):
    """Row 0 of S names a column row 0 of A does not have.  The kernels treat it as data: the flag is raised
    and the call fails with P untouched; the host form refuses it too.  Column 9 of a 5-row S is out of
    range for the graph."""
    c = K.inconsistent_case()
    n = len(c.mark)
    Am = NumpyCSR(*c.A)
    S = SSS_IMAT(n, n, len(c.S[1]), iptr(c.S[0]), iptr(c.S[1]), None)
    P, keep = _sentinel_p(n)
    passes = C.c_int(-7)
    rc = A.lib().sss_hip_interp_mpass(C.byref(Am.mat), C.byref(S), iptr(c.mark), C.byref(P), MP.TRUNC, C.byref(passes))
    assert rc == ERROR_DATA_STRUCTURE
    assert "strong column absent" in capfd.readouterr().err
    assert _untouched(P, keep, n) and passes.value == -7
    with pytest.raises(RuntimeError) as e:
        A.interp_mpass(c.A, c.S, c.mark, MP.TRUNC, device=True)
    assert e.value.rc == rc and e.value.untouched
    with pytest.raises(RuntimeError) as e:
        A.interp_mpass(c.A, c.S, c.mark, MP.TRUNC)
    assert e.value.rc == rc
    bad = np.where(c.S[1] == 3, 9, c.S[1]).astype(np.int32)
    Sb = SSS_IMAT(n, n, len(bad), iptr(c.S[0]), iptr(bad), None)
    S2, rp = _sentinel_s2()
    assert A.lib().sss_hip_agg_graph(C.byref(Sb), iptr(c.mark), C.byref(S2)) == ERROR_DATA_STRUCTURE
    assert "index out of range" in capfd.readouterr().err and _untouched_s2(S2, rp)


@pytest.fixture(scope="module")
def agg_16():
    with quiet_ctx():
        H = A.Hierarchy(R.matrix("p7_16"), R.pars(MP.AGG, MP.STD))
    yield H
    H.close()


def test_parity_mode_solve_is_the_oracles(agg_16):
    H = agg_16
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


def test_throughput_mode_pcg_converges(agg_16):
    H = agg_16
    n = H.level(0).A.num_rows
    D = A.DeviceHierarchy(H, smoother="hybrid", coarse="direct")
    try:
        D.upload(0, "b", np.random.default_rng(1).standard_normal(n))
        D.upload(0, "x", np.zeros(n))
        its, hist = D.pcg(1e-6, 100)
    finally:
        D.close()
    print(f"p7_16 cs_type 4: pcg {its} iterations, {hist[-1]:.3e}")
    assert hist[-1] < 1e-6 and its < 100


def _infos(D, levels):
    names = [f[0] for f in SSS_HIP_LEVEL_INFO._fields_]
    return [tuple(getattr(D.level_info(l), f) for f in names) for l in range(levels)]


def test_mirror_refresh_equals_a_fresh_mirror():
    M = RC.matrix("p7_16")
    with quiet_ctx():
        H = A.Hierarchy(M, R.pars(MP.AGG, MP.STD))
    n = M.num_rows
    b = np.random.default_rng(2).standard_normal(n)
    D = A.DeviceHierarchy(H, smoother="hybrid", coarse="direct")
    F = None
    try:
        M2 = RC.drifted(M, 0.3, 0.0)   # keeps the new values' buffers alive
        H.refresh(M2.mat)
        D.refresh()
        F = A.DeviceHierarchy(H, smoother="hybrid", coarse="direct")
        assert _infos(D, H.num_levels) == _infos(F, H.num_levels)
        xs = []
        for E in (D, F):
            E.upload(0, "b", b)
            E.upload(0, "x", np.zeros(n))
            E.cycle()
            xs.append(E.download(0, "x"))
        assert np.array_equal(xs[0].view(np.uint64), xs[1].view(np.uint64))
    finally:
        D.close()
        if F is not None:
            F.close()
        H.close()
