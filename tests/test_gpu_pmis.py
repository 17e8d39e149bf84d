"""GPU: the PMIS C/F split on the device (sss_hip_pmis, amg_amd/csrc/sss_pmis.hip) against the host
split and the numpy restatement of the rule (tests/pmis_restatement.py): marks, C count and rounds equal
on every matrix, hierarchy level and hand-built S, with every lane-group width; whole setups with the
device split forced build the hierarchy the host split builds (digest over A, P, R, cfmark); the solve
phase runs a PMIS hierarchy in parity mode (bitwise the oracle) and in throughput mode; the error path."""
from __future__ import annotations

import ctypes as C
import hashlib

import numpy as np
import pytest

import amg_amd as A
import pmis_restatement as R
from amg_amd._native import SSS_IMAT, iptr
from conftest import device_mode_oracle_opts, oracle_solve, quiet_ctx

pytestmark = pytest.mark.gpu

S_NAMES = ["p7_12", "p7_24", "a27_8", "circuit3000", "bus", "n1", "empty_row", "lambda0_neighbour",
           "nobody_depends", "long_row_700", "n257", "n1025", "n4097_long"]


def _check(name, rp, ci):
    want = R.pmis_restated(rp, ci)
    host = A.pmis(rp, ci)
    dev = A.pmis(rp, ci, device=True)
    assert np.array_equal(dev[0], want[0]) and np.array_equal(dev[0], host[0]), name
    assert dev[1:] == want[1:] == host[1:], (name, dev[1:], host[1:], want[1:])
    R.check_invariants(rp, ci, dev[0], dev[1])


@pytest.mark.parametrize("name", S_NAMES)
def test_device_split_equals_host_and_restatement(name, quiet):
    _check(name, *R.all_s(quiet)[name])


def test_device_split_on_hierarchy_levels(quiet):
    names = [k for k in R.all_s(quiet) if "_level" in k]
    assert len(names) >= 6
    for name in names:
        _check(name, *R.all_s(quiet)[name])


@pytest.mark.parametrize("lanes", ["1", "4", "16", "64"])
def test_every_lane_group_width(lanes, quiet, monkeypatch):
    """The lane group is chosen from the average row length; here each width walks short rows, a
    700-entry row, rows of up to 30 and a coarse level, whatever their average."""
    monkeypatch.setenv("SSS_HIP_PMIS_LANES", lanes)
    for name in ["a27_8", "long_row_700", "n4097_long", "n257", "p7_24_level1", "circuit3000_level2", "empty_row", "n1"]:
        _check(name, *R.all_s(quiet)[name])


def _digest(H) -> str:
    h = hashlib.sha256()
    for l in range(H.num_levels):
        L = H.level(l)
        mats = [L.A] if l == H.num_levels - 1 else [L.A, L.P, L.R]
        for M in mats:
            h.update(np.array([M.num_rows, M.num_cols, M.num_nnzs], np.int64).tobytes())
            for arr in A.csr_arrays(M):
                h.update(arr.tobytes())
        if l < H.num_levels - 1:
            h.update(np.ctypeslib.as_array(L.cfmark.d, shape=(L.A.num_rows,)).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("case", ["p7_24", "a27_12", "circuit60000"])
def test_setup_with_device_split_same_hierarchy(case, monkeypatch, capfd):
    M = R.matrix(case)
    monkeypatch.setenv("SSS_SETUP_TIMING", "1")
    monkeypatch.setenv("SSS_SETUP_GPU_PMIS", "0")
    with quiet_ctx():
        H = A.Hierarchy(M, R.pars())
    d_host, levels = _digest(H), H.num_levels
    H.close()
    err = capfd.readouterr().err
    # one split per level that was coarsened (the last attempt may be discarded by the level loop)
    assert err.count("host split") >= levels - 1 and "device split" not in err
    monkeypatch.setenv("SSS_SETUP_GPU_PMIS", "1")
    monkeypatch.setenv("SSS_SETUP_GPU_PMIS_MIN", "0")
    with quiet_ctx():
        H = A.Hierarchy(M, R.pars())
    d_dev = _digest(H)
    H.close()
    err = capfd.readouterr().err
    assert err.count("device split") >= levels - 1 and "host split" not in err
    assert d_dev == d_host


@pytest.fixture(scope="module")
def pmis_hiers():
    hs = {}
    yield hs
    for H in hs.values():
        H.close()


def _hier(gen, hs):
    if gen not in hs:
        with quiet_ctx():
            hs[gen] = A.Hierarchy(R.matrix(gen), R.pars())
    return hs[gen]


@pytest.mark.parametrize("gen", ["bus", "p7_24", "a27_12"])
def test_pmis_hierarchy_parity_mode(gen, pmis_hiers):
    H = _hier(gen, pmis_hiers)
    n = H.level(0).A.num_rows
    rtn, rel_r, _ = oracle_solve(H, np.ones(n), x_r := np.ones(n))
    D = A.DeviceHierarchy(H, smoother="exact", coarse="krylov")
    try:
        D.upload(0, "b", np.ones(n))
        D.upload(0, "x", np.ones(n))
        rel_g = []
        for _ in range(len(rel_r)):
            D.cycle()
            rel_g.append(D.residual_norm() / np.sqrt(n))
        x_g = D.download(0, "x")
    finally:
        D.close()
    assert rel_r[-1] < H.pars.tol
    assert np.array_equal(x_g.view(np.uint64), x_r.view(np.uint64))
    assert np.allclose(rel_g, rel_r, rtol=1e-13, atol=0)


@pytest.mark.parametrize("gen", ["bus", "p7_24", "a27_12"])
def test_pmis_hierarchy_throughput_mode(gen, pmis_hiers):
    H = _hier(gen, pmis_hiers)
    n = H.level(0).A.num_rows
    mode = dict(smoother="hybrid", coarse="direct")
    rtn, rel_o, _ = oracle_solve(H, np.ones(n), np.zeros(n), **device_mode_oracle_opts(H, **mode))
    assert rel_o[-1] < H.pars.tol
    D = A.DeviceHierarchy(H, **mode)
    try:
        D.upload(0, "b", np.ones(n))
        D.upload(0, "x", np.zeros(n))
        rel = []
        while len(rel) < 100:   # the V-cycle loop, on to the PCG's tolerance
            D.cycle()
            rel.append(D.residual_norm() / np.sqrt(n))
            if rel[-1] < 1e-8:
                break
        D.upload(0, "x", np.zeros(n))
        its, hist = D.pcg(1e-8, 100)
    finally:
        D.close()
    to_tol = 1 + next(k for k, r in enumerate(rel) if r < H.pars.tol)
    print(f"{gen}: oracle {len(rel_o)} its, V-cycle loop {to_tol} to tol / {len(rel)} to 1e-8, pcg {its}")
    assert rel[-1] < 1e-8
    assert hist[-1] < 1e-8
    assert its <= len(rel)
    assert to_tol <= len(rel_o) + 2


def test_error_path_no_rows():
    """num_rows 0: an error code, mark untouched, nothing launched (the check precedes every HIP call)."""
    rp = np.zeros(1, np.int32)
    ci = np.zeros(1, np.int32)
    S = SSS_IMAT(0, 0, 0, iptr(rp), iptr(ci), None)
    mark = np.full(4, -7, np.int32)
    nc, rounds = C.c_int(-5), C.c_int(-5)
    rc = A.lib().sss_hip_pmis(C.byref(S), iptr(mark), C.byref(nc), C.byref(rounds))
    assert rc < 0
    assert (mark == -7).all() and nc.value == -5 and rounds.value == -5
