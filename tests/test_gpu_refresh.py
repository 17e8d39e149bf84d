"""GPU: the refresh of a set-up hierarchy for new operator values -- the values-only
Galerkin product on the device (sss_hip_rap_values, amg_amd/csrc/sss_rap.hip) against sss_hip_rap with
every table size and host rows, SSS_amg_refresh with the device products against the all-host
refresh, the refreshed mirror (sss_hip_hier_refresh) against a mirror newly created from the
refreshed hierarchy, and the drop-in solve path across a refresh.  Everything is compared on bits."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import amg_amd as A
import refresh_cases as RC
from amg_amd._native import SSS_VEC, dptr
from conftest import quiet_ctx

pytestmark = pytest.mark.gpu

ERROR_DATA_STRUCTURE = -21
_levels = {}


def _device_products(name):
    """(hierarchy, [sss_hip_rap(R_l, A_l, P_l) of every level]) of the named matrix, built once."""
    if name not in _levels:
        H = RC.hierarchy(RC.matrix(name))
        prods = []
        for l in range(H.num_levels - 1):
            L = H.level(l)
            Cg = A.SSS_MAT()
            assert A.lib().sss_hip_rap(C.byref(L.R), C.byref(L.A), C.byref(L.P), C.byref(Cg)) == 0
            prods.append(Cg)
        _levels[name] = (H, prods)
    return _levels[name]


@pytest.mark.parametrize("name", ["p7_32", "a27_20", "circuit60000", "bus"])
@pytest.mark.parametrize("cfgs", ["4", "2", "1", "0"])
def test_values_only_product_is_the_device_product(name, cfgs, monkeypatch):
    H, prods = _device_products(name)
    monkeypatch.setenv("SSS_HIP_RAP_CFGS", cfgs)   # fewer device tables: longer rows on the host
    for l, Cg in enumerate(prods):
        L = H.level(l)
        Cv = RC.pattern_copy(Cg)
        A.rap_values(L.R, L.A, L.P, Cv.mat, device=True)
        assert RC.same_bits(Cv.mat, Cg), (name, cfgs, l)


@pytest.mark.parametrize("cfgs", ["4", "0"])
def test_values_only_product_signed_zeros(cfgs, monkeypatch):
    monkeypatch.setenv("SSS_HIP_RAP_CFGS", cfgs)
    R, Am, P = RC.signed_zero_case()
    Ch = RC.host_rap(R.mat, Am.mat, P.mat)
    try:
        Cv = RC.pattern_copy(Ch)
        A.rap_values(R.mat, Am.mat, P.mat, Cv.mat, device=True)
        assert not np.signbit(Cv.v[0]) and np.signbit(Cv.v[1]) and Cv.v[1] == 0.0
        assert RC.same_bits(Cv.mat, Ch)
    finally:
        A.lib().SSS_mat_destroy(C.byref(Ch))


@pytest.mark.parametrize("cfgs", ["4", "0"])
def test_values_only_product_missing_column(cfgs, monkeypatch):
    monkeypatch.setenv("SSS_HIP_RAP_CFGS", cfgs)
    H, prods = _device_products("p7_32")
    L = H.level(0)
    Cv = RC.pattern_copy(prods[0], fill=7.0)
    row = 5
    k = int(Cv.rp[row]) + 1
    unused = sorted(set(range(Cv.mat.num_rows)) - set(Cv.ci[Cv.rp[row]:Cv.rp[row + 1]].tolist()))
    Cv.ci[k] = unused[0]
    with pytest.raises(RuntimeError) as e:
        A.rap_values(L.R, L.A, L.P, Cv.mat, device=True)
    assert e.value.rc == ERROR_DATA_STRUCTURE
    assert np.all(Cv.v == 7.0)


@pytest.mark.parametrize("name", ["p7_32", "a27_20", "circuit60000"])
def test_refresh_with_device_products_is_the_host_refresh(name, monkeypatch, capfd):
    M = RC.matrix(name)
    N = RC.drifted(M, 0.3, 0.0)
    H = RC.hierarchy(M)
    monkeypatch.setenv("SSS_SETUP_GPU_RAP", "0")
    H.refresh(N.mat)
    d_host = RC.digest(H)
    H.refresh(M)
    assert RC.digest(H) != d_host
    monkeypatch.setenv("SSS_SETUP_GPU_RAP", "1")
    monkeypatch.setenv("SSS_SETUP_GPU_RAP_MIN", "0")
    monkeypatch.setenv("SSS_SETUP_GPU_RAP_MAXROW", "100000")
    monkeypatch.setenv("SSS_SETUP_TIMING", "1")
    capfd.readouterr()
    H.refresh(N.mat)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[refresh]")]
    assert len(lines) == H.num_levels - 1 and all(" device " in ln for ln in lines), lines
    assert RC.digest(H) == d_host
    H.close()


MODES = [dict(smoother="exact", coarse="krylov"), dict(smoother="hybrid", coarse="direct")]


def _two_cycles(D, n):
    D.upload(0, "x", np.zeros(n))
    D.cycle()
    D.cycle()
    return D.download(0, "x"), D.residual_norm()


def _info(D, nl):
    return [tuple(getattr(i, f) for f, _ in i._fields_) for i in (D.level_info(l) for l in range(nl))]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_refreshed_mirror(D, H, M, N, b):
    """D mirrors H (set up on M, b uploaded): across H.refresh(N) + D.refresh() it is the mirror newly
    created from the refreshed H, and back on M's values it is what it was."""
    n, nl = M.num_rows, H.num_levels
    x_old, r_old = _two_cycles(D, n)   # (the graphs of the old operators are captured by now)
    H.refresh(N.mat)
    D.refresh()
    assert np.array_equal(_bits(D.download(0, "b")), _bits(b))   # the level-0 b stayed
    x_new, r_new = _two_cycles(D, n)
    its, hist = None, None
    D.upload(0, "x", np.zeros(n))
    its, hist = D.pcg(1e-10, 30)
    F = A.DeviceHierarchy(H, **D.kw)
    try:
        F.upload(0, "b", b)
        x_f, r_f = _two_cycles(F, n)
        F.upload(0, "x", np.zeros(n))
        its_f, hist_f = F.pcg(1e-10, 30)
        assert _info(D, nl) == _info(F, nl)
    finally:
        F.close()
    assert np.array_equal(_bits(x_new), _bits(x_f))
    assert _bits(np.array([r_new]))[0] == _bits(np.array([r_f]))[0]
    assert its == its_f and np.array_equal(_bits(hist), _bits(hist_f))
    assert not np.array_equal(x_new, x_old)
    H.refresh(M)
    D.refresh()
    x_back, r_back = _two_cycles(D, n)
    assert np.array_equal(_bits(x_back), _bits(x_old)) and r_back == r_old


@pytest.mark.parametrize("name", ["p7_16", "p7_24", "a27_8", "bus", "circuit3000"])
@pytest.mark.parametrize("amp,shift", [(0.3, 0.0), (0.9, 0.1)])
@pytest.mark.parametrize("mode", [0, 1])
def test_refreshed_mirror_is_a_new_mirror(name, amp, shift, mode):
    M = RC.matrix(name)
    N = RC.drifted(M, amp, shift)
    H = RC.hierarchy(M)
    kw = dict(MODES[mode], graph=1)
    D = A.DeviceHierarchy(H, **kw)
    D.kw = kw
    try:
        b = np.random.default_rng(1).standard_normal(M.num_rows)
        D.upload(0, "b", b)
        _check_refreshed_mirror(D, H, M, N, b)
    finally:
        D.close()
        H.close()


def test_refreshed_mirror_from_the_overlapped_setup():
    M = RC.matrix("p7_24")
    N = RC.drifted(M, 0.3, 0.0)
    kw = dict(MODES[1], graph=1)
    with quiet_ctx():
        D = A.DeviceHierarchy(None, setup_from=M, **kw)
    D.kw = kw
    try:
        b = np.random.default_rng(1).standard_normal(M.num_rows)
        D.upload(0, "b", b)
        _check_refreshed_mirror(D, D.H, M, N, b)
    finally:
        D.close()
        D.H.close()


def _dropin_solve(H, b):
    n = len(b)
    x = np.zeros(n)
    with quiet_ctx():
        rtn = A.lib().SSS_amg_solve(C.byref(H.mg), C.byref(SSS_VEC(n, dptr(x))), C.byref(SSS_VEC(n, dptr(b))))
    return rtn.nits, x


@pytest.mark.parametrize("name", ["p7_16", "bus"])
def test_dropin_solve_across_a_refresh(name):
    """SSS_amg_solve builds and registers the mirror; SSS_amg_refresh refreshes it with the hierarchy."""
    M = RC.matrix(name)
    N = RC.drifted(M, 0.3, 0.0)
    b = np.random.default_rng(1).standard_normal(M.num_rows)
    H = RC.hierarchy(M)
    its0, x0 = _dropin_solve(H, b)
    H.refresh(N.mat)
    its1, x1 = _dropin_solve(H, b)
    G = RC.hierarchy(M)      # a hierarchy with no mirror yet: the solve after its refresh builds a new one
    G.refresh(N.mat)
    its2, x2 = _dropin_solve(G, b)
    assert its1 == its2 and np.array_equal(_bits(x1), _bits(x2))
    assert not np.array_equal(x0, x1)
    H.close()
    G.close()
