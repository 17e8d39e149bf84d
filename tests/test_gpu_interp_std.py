"""GPU: the standard interpolation's pattern and weights on the device (sss_hip_std_pattern,
sss_hip_interp_std, amg_amd/csrc/sss_interp.hip) against the host: arrays equal and values bit for bit on
every case of tests/interp_std_cases.py, with the default truncation and with none, with every lane-group
width, with the per-row tables in LDS and in global memory; whole setups with the device path forced
build the hierarchy the host path builds (digest over A, P, R, cfmark); the error paths."""
from __future__ import annotations

import ctypes as C
import hashlib
import re

import numpy as np
import pytest

import amg_amd as A
import interp_std_cases as K
import pmis_restatement as R
from amg_amd._native import SSS_IMAT, SSS_MAT, NumpyCSR, iptr
from conftest import quiet_ctx

pytestmark = pytest.mark.gpu

NATURAL = [f"{n}_{t}" for t in ["rs", "pmis"] for n in K.NATURAL]
HAND = ["star20", "star130", "n1_c", "ispt_row", "f_only_neighbours", "f_in_nobodys_s"]
SMALL = ["n1_c", "ispt_row", "f_only_neighbours", "f_in_nobodys_s"]
_host = {}


def host_weights(name, c, trunc):
    """The host result of a case, computed once."""
    if (name, trunc) not in _host:
        with quiet_ctx():
            _host[name, trunc] = A.interp_std(c.A, c.S, c.mark, c.P, trunc)
    return _host[name, trunc]


def check_pattern(name, c):
    got = A.std_pattern(*c.S, c.mark, device=True)
    assert np.array_equal(got[0], c.P[0]) and np.array_equal(got[1], c.P[1]), name


def check_weights(name, c, trunc):
    got = A.interp_std(c.A, c.S, c.mark, c.P, trunc, device=True)
    K.assert_same_p(got, host_weights(name, c, trunc), (name, trunc))


def level_names(cases):
    return [k for k in cases if "_level" in k]


@pytest.mark.parametrize("name", NATURAL + HAND)
def test_device_pattern_equals_host(name, quiet):
    check_pattern(name, K.all_cases(quiet)[name])


def test_device_pattern_on_hierarchy_levels(quiet):
    cases = K.all_cases(quiet)
    assert len(level_names(cases)) >= 8
    for name in level_names(cases):
        check_pattern(name, cases[name])


@pytest.mark.parametrize("trunc", [K.TRUNC, 0.0])
@pytest.mark.parametrize("name", NATURAL + HAND)
def test_device_weights_equal_host(name, trunc, quiet):
    check_weights(name, K.all_cases(quiet)[name], trunc)


@pytest.mark.parametrize("trunc", [K.TRUNC, 0.0])
def test_device_weights_on_hierarchy_levels(trunc, quiet):
    cases = K.all_cases(quiet)
    for name in level_names(cases):
        check_weights(name, cases[name], trunc)


@pytest.mark.parametrize("lanes", ["1", "4", "16", "64"])
def test_every_lane_group_width(lanes, quiet, monkeypatch):
    """The lane group is chosen from the average row of S; here each width walks short rows, the longest
    natural rows, a coarse PMIS level, a 403-entry row and the small cases, whatever their average."""
    monkeypatch.setenv("SSS_HIP_INTERP_LANES", lanes)
    cases = K.all_cases(quiet)
    for name in ["a27_8_rs", "p7_24_rs_level3", "circuit3000_pmis_level2", "star20"] + SMALL:
        check_pattern(name, cases[name])
        for trunc in [K.TRUNC, 0.0]:
            check_weights(name, cases[name], trunc)


def global_rows(err, step):
    m = re.findall(rf"device {step},.* (\d+) rows on global tables", err)
    assert len(m) == 1, err
    return int(m[0])


@pytest.mark.parametrize("name,slots", [("star130", None), ("star20", "64"), ("p7_24_rs_level2", "64")])
def test_global_table_path(name, slots, quiet, monkeypatch, capfd):
    """Rows whose candidate bound exceeds the LDS table take a table in global memory inside the same
    call: star(130)'s 16903-entry row with nothing forced, the others with the LDS table lowered."""
    monkeypatch.setenv("SSS_SETUP_TIMING", "1")
    if slots:
        monkeypatch.setenv("SSS_HIP_INTERP_LDS_SLOTS", slots)
    c = K.all_cases(quiet)[name]
    host = [host_weights(name, c, t) for t in [K.TRUNC, 0.0]]
    capfd.readouterr()
    check_pattern(name, c)
    assert global_rows(capfd.readouterr().err, "pattern") > 0
    for trunc, want in zip([K.TRUNC, 0.0], host):
        check_weights(name, c, trunc)
        assert global_rows(capfd.readouterr().err, "weights") > 0


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


@pytest.mark.parametrize("cs", [K.RS, K.PMIS])
@pytest.mark.parametrize("case", ["p7_24", "a27_12", "circuit60000"])
def test_setup_with_device_interpolation_same_hierarchy(case, cs, monkeypatch, capfd):
    M = R.matrix(case)
    monkeypatch.setenv("SSS_SETUP_TIMING", "1")
    monkeypatch.setenv("SSS_SETUP_GPU_INTERP", "0")
    with quiet_ctx():
        H = A.Hierarchy(M, R.pars(cs, K.STD))
    d_host, levels = _digest(H), H.num_levels
    H.close()
    err = capfd.readouterr().err
    # one pattern and one weight computation per coarsened level (the level loop may discard the last)
    for step in ["pattern", "weights"]:
        assert err.count(f"host {step}") >= levels - 1 and f"device {step}" not in err
    monkeypatch.setenv("SSS_SETUP_GPU_INTERP", "1")
    monkeypatch.setenv("SSS_SETUP_GPU_INTERP_MIN", "0")
    with quiet_ctx():
        H = A.Hierarchy(M, R.pars(cs, K.STD))
    d_dev = _digest(H)
    H.close()
    err = capfd.readouterr().err
    for step in ["pattern", "weights"]:
        assert err.count(f"device {step}") >= levels - 1 and f"host {step}" not in err
    assert d_dev == d_host


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
    c = K.all_cases(quiet)["f_in_nobodys_s"]
    n = len(c.mark)
    Am = NumpyCSR(*c.A)
    lib = A.lib()
    for rows, mark in [(0, iptr(c.mark)), (n, None)]:
        S = SSS_IMAT(rows, rows, len(c.S[1]), iptr(c.S[0]), iptr(c.S[1]), None)
        P, keep = _sentinel_p(n)
        assert lib.sss_hip_std_pattern(C.byref(S), mark, 2, C.byref(P)) < 0
        assert _untouched(P, keep, n)
        assert lib.sss_hip_interp_std(C.byref(Am.mat), C.byref(S), mark, C.byref(P), K.TRUNC) < 0
        assert _untouched(P, keep, n)


def test_inconsistent_s_is_an_error_code(capfd):
    """Row 0 of S names a column row 0 of A does not have.  The kernels treat it as data: the search of
    the row finds nothing, the flag is raised, and the call fails with P untouched."""
    c = K.inconsistent_case()
    n = len(c.mark)
    Am = NumpyCSR(*c.A)
    S = SSS_IMAT(n, n, len(c.S[1]), iptr(c.S[0]), iptr(c.S[1]), None)
    lib = A.lib()
    P = lib.SSS_mat_struct_create(n, int((c.mark == K.CGPT).sum()), len(c.P[1]))
    C.memmove(P.row_ptr, c.P[0].ctypes.data, c.P[0].nbytes)
    C.memmove(P.col_idx, c.P[1].ctypes.data, c.P[1].nbytes)
    before = (P.num_rows, P.num_cols, P.num_nnzs, C.addressof(P.row_ptr.contents), C.addressof(P.col_idx.contents),
              C.addressof(P.val.contents))
    rc = lib.sss_hip_interp_std(C.byref(Am.mat), C.byref(S), iptr(c.mark), C.byref(P), K.TRUNC)
    assert rc < 0
    assert "strong column absent" in capfd.readouterr().err
    after = (P.num_rows, P.num_cols, P.num_nnzs, C.addressof(P.row_ptr.contents), C.addressof(P.col_idx.contents),
             C.addressof(P.val.contents))
    assert after == before
    rp, ci, v = A.csr_arrays(P)
    assert np.array_equal(rp, c.P[0]) and np.array_equal(ci, c.P[1]) and (v == 0).all()
    lib.SSS_mat_destroy(C.byref(P))
    with pytest.raises(RuntimeError) as e:
        A.interp_std(c.A, c.S, c.mark, c.P, K.TRUNC, device=True)
    assert e.value.rc == rc
