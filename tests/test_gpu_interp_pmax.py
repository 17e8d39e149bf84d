"""GPU: the truncation with the cap on the entries per row of P on the device (sss_hip_interp_trunc and the
tail of the three device interpolations, amg_amd/csrc/sss_interp.hip) against the host's,
arrays equal and values bit for bit: on the untruncated P of every standard, extended+i and multipass case
and on the hand-built rows, with every lane-group width and with the width the chooser picks; the device
interpolations under SSS_SETUP_PMAX; whole setups forced to the device; the error paths; the solve phase
on a capped PMIS + extended+i hierarchy in parity mode (bitwise the oracle) and in throughput mode; the
mirror's refresh."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import amg_amd as A
import interp_std_cases as K
import mpass_cases as MP
import pmax_cases as PC
import pmis_restatement as R
import refresh_cases as RC
from amg_amd._native import SSS_HIP_LEVEL_INFO, SSS_MAT, iptr
from conftest import oracle_solve, quiet_ctx

pytestmark = pytest.mark.gpu

ERROR_INPUT_PAR = -12   # include/sss_amg.h
_host = {}


@pytest.fixture(autouse=True)
def _cap_off(monkeypatch):
    monkeypatch.delenv("SSS_SETUP_PMAX", raising=False)


def inputs(quiet):
    """name -> untruncated P: every case of the CPU test, and the hand-built rows (the tie, the lost sign)."""
    out = {(t, n): PC.untruncated(t, n, quiet) for t, n in PC.input_names(quiet)}
    out[0, "hand"] = PC.hand_p()
    return out


def host_trunc(key, P, eps, pmax):
    """The host's result, computed once and shared by the tests."""
    if (key, eps, pmax) not in _host:
        _host[key, eps, pmax] = A.interp_trunc(P[:3], P[3], eps, pmax)
    return _host[key, eps, pmax]


def check_all(quiet, pmaxes):
    capped_rows = 0
    for key, P in inputs(quiet).items():
        for eps in PC.EPS:
            for pmax in pmaxes:
                want = host_trunc(key, P, eps, pmax)
                K.assert_same_p(A.interp_trunc(P[:3], P[3], eps, pmax, device=True), want, (key, eps, pmax))
                capped_rows += int((np.diff(want[0]) == pmax).sum()) if pmax else 0
    return capped_rows


@pytest.mark.parametrize("lanes", ["1", "4", "16", "64"])
def test_device_truncation_equals_host_at_every_lane_width(lanes, quiet, monkeypatch):
    """Each width walks the short rows of the stencils, the rows of hundreds of entries of the coarse levels
    and of star20, the 16,903-entry row of star130, the hand-built tie and lost-sign rows."""
    monkeypatch.setenv("SSS_HIP_INTERP_LANES", lanes)
    assert check_all(quiet, PC.PMAX) > 1000


def test_device_truncation_with_the_chosen_width_and_without_cap(quiet, monkeypatch, capfd):
    """Nothing forced: the width comes from the mean row of P (up to 4 entries one lane, up to 16 four, up to
    64 sixteen, else 64): one lane for the stars, whose mean row has 3 entries although one has 16,903.
    pmax 0 runs the uncapped kernels; a cap as long as the longest row changes nothing."""
    monkeypatch.delenv("SSS_HIP_INTERP_LANES", raising=False)
    check_all(quiet, [0, 4])
    monkeypatch.setenv("SSS_SETUP_TIMING", "1")
    capfd.readouterr()
    widths = set()
    for itype, name in [(PC.EXTI, "star130"), (PC.EXTI, "p7_24_pmis_level1"), (PC.STD, "p7_24_rs_level3")]:
        P = PC.untruncated(itype, name, quiet)
        longest, mean = int(np.diff(P[0]).max()), len(P[1]) / (len(P[0]) - 1)
        lanes = 1 if mean <= 4 else 4 if mean <= 16 else 16 if mean <= 64 else 64
        widths.add(lanes)
        got = A.interp_trunc(P[:3], P[3], K.TRUNC, longest, device=True)
        K.assert_same_p(got, host_trunc((itype, name), P, K.TRUNC, 0), name)
        assert f"cap {longest} at {lanes} lanes per row" in capfd.readouterr().err
    assert len(widths) >= 2


@pytest.mark.parametrize("pmax", ["2", "4"])
def test_device_interpolations_take_the_cap(pmax, quiet, monkeypatch):
    """The tail the three device interpolations share reads SSS_SETUP_PMAX as the host's truncation does."""
    monkeypatch.setenv("SSS_SETUP_PMAX", pmax)
    for name in ["p7_12_pmis", "star20"]:
        c = K.all_cases(quiet)[name]
        for fn in (A.interp_std, A.interp_exti):
            for trunc in PC.EPS:
                with quiet():
                    want = fn(c.A, c.S, c.mark, c.P, trunc)
                assert np.diff(want[0]).max() <= int(pmax)
                K.assert_same_p(fn(c.A, c.S, c.mark, c.P, trunc, device=True), want, (name, fn.__name__, trunc, pmax))
    for name in ["p7_12", "mstar12"]:
        c = MP.all_cases(quiet)[name]
        for trunc in PC.EPS:
            with quiet():
                want = A.interp_mpass(c.A, c.S, c.mark, trunc)
            assert np.diff(want[0]).max() <= int(pmax)
            got = A.interp_mpass(c.A, c.S, c.mark, trunc, device=True)
            K.assert_same_p(got[:4], want[:4], (name, trunc, pmax))
            assert got[4] == want[4]


@pytest.mark.parametrize("cs,interp", [(3, 2), (3, 3), (4, 2)])
def test_setup_on_the_device_same_capped_hierarchy(cs, interp, monkeypatch, capfd):
    M = R.matrix("p7_16")
    monkeypatch.setenv("SSS_SETUP_PMAX", "4")
    monkeypatch.setenv("SSS_SETUP_TIMING", "1")
    for v in ("SSS_SETUP_GPU_AGG", "SSS_SETUP_GPU_INTERP", "SSS_SETUP_GPU_PMIS"):
        monkeypatch.setenv(v, "0")
    with quiet_ctx():
        H = A.Hierarchy(M, R.pars(cs, interp))
    d_host, levels = RC.digest(H), H.num_levels
    longest = max(int(np.diff(A.csr_arrays(H.level(l).P)[0]).max()) for l in range(levels - 1))
    H.close()
    assert "device" not in capfd.readouterr().err
    for v in ("SSS_SETUP_GPU_AGG", "SSS_SETUP_GPU_INTERP", "SSS_SETUP_GPU_PMIS"):
        monkeypatch.setenv(v, "1")
        monkeypatch.setenv(v + "_MIN", "0")
    with quiet_ctx():
        H = A.Hierarchy(M, R.pars(cs, interp))
    d_dev = RC.digest(H)
    H.close()
    err = capfd.readouterr().err
    assert err.count(", cap 4 at ") >= levels - 1, err   # every level's interpolation ran on the device, capped
    assert levels >= 3 and longest <= 4 and d_dev == d_host


def _sentinel_p():
    rp = np.array([0, 2, 3, 4], np.int32)
    ci = np.array([0, 1, 1, 0], np.int32)
    v = np.array([0.5, -7.0, 1.0, 1.0])
    return SSS_MAT(3, 2, 4, iptr(rp), iptr(ci), v.ctypes.data_as(C.POINTER(C.c_double))), (rp, ci, v)


def _untouched(P, keep):
    rp, ci, v = keep
    return (P.num_rows, P.num_cols, P.num_nnzs) == (3, 2, 4) and rp.tolist() == [0, 2, 3, 4] and ci.tolist() == [0, 1, 1, 0] \
        and v.tolist() == [0.5, -7.0, 1.0, 1.0] and C.addressof(P.row_ptr.contents) == rp.ctypes.data \
        and C.addressof(P.col_idx.contents) == ci.ctypes.data and C.addressof(P.val.contents) == v.ctypes.data


def test_error_paths_nothing_launched(monkeypatch, capfd):
    """pmax < 0 and a NULL P: ERROR_INPUT_PAR, the sentinel P untouched, and no timing line (the checks
    precede every HIP call)."""
    monkeypatch.setenv("SSS_SETUP_TIMING", "1")
    fn = A.lib().sss_hip_interp_trunc
    P, keep = _sentinel_p()
    assert fn(C.byref(P), 0.2, -1) == ERROR_INPUT_PAR and _untouched(P, keep)
    assert fn(None, 0.2, 4) == ERROR_INPUT_PAR and _untouched(P, keep)
    keep[0][0] = 1   # misshapen: the row pointers do not start at 0
    assert fn(C.byref(P), 0.2, 4) == ERROR_INPUT_PAR
    keep[0][0] = 0
    assert _untouched(P, keep) and "truncation" not in capfd.readouterr().err


# ---------------------------------------------------------------- the solve phase on a capped hierarchy
@pytest.fixture(scope="module")
def capped_16():
    mp = pytest.MonkeyPatch()
    mp.setenv("SSS_SETUP_PMAX", "4")
    try:
        with quiet_ctx():
            H = A.Hierarchy(R.matrix("p7_16"), R.pars(3, 3))
    finally:
        mp.undo()
    yield H
    H.close()


def test_parity_mode_solve_is_the_oracles(capped_16):
    H = capped_16
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


def test_throughput_mode_pcg_converges(capped_16):
    H = capped_16
    n = H.level(0).A.num_rows
    D = A.DeviceHierarchy(H, smoother="hybrid", coarse="direct")
    try:
        D.upload(0, "b", np.random.default_rng(1).standard_normal(n))
        D.upload(0, "x", np.zeros(n))
        its, hist = D.pcg(1e-6, 100)
    finally:
        D.close()
    print(f"p7_16 PMIS + extended+i, cap 4: pcg {its} iterations, {hist[-1]:.3e}")
    assert hist[-1] < 1e-6 and its < 100


def _infos(D, levels):
    names = [f[0] for f in SSS_HIP_LEVEL_INFO._fields_]
    return [tuple(getattr(D.level_info(l), f) for f in names) for l in range(levels)]


def test_mirror_refresh_equals_a_fresh_mirror(monkeypatch):
    M = RC.matrix("p7_16")
    monkeypatch.setenv("SSS_SETUP_PMAX", "4")
    with quiet_ctx():
        H = A.Hierarchy(M, R.pars(3, 3))
    monkeypatch.delenv("SSS_SETUP_PMAX")
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
