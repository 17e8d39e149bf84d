"""GPU: the kernels of every storage format at the format's own limits (format_cases.py).

The rest of the suite reaches the formats through the hierarchies of a few matrices and sees
whatever dictionary fills and row widths those produce.  Here every case is uploaded through
sss_hip_host_spmv_enc / sss_hip_host_level_step with a chosen encoding; what the upload chose
(format bits, row width, shift, bases, blocks) is asserted first, so no case can pass by landing on
another format, and then:

  SpMV        the four ops as uint64 against ora_mv_mxy / ora_mv_amxpy / ora_mv_acc (ACC with its row
              cap below and above n), for every encoding a case lists;
  level step  exact GS-CF on the bipartite cases (both passes must be range passes), C/F-Jacobi, and
              two-stage with 1 and 2 inner steps (the split copies' formats asserted), with 1 and 2
              sweeps, pre and post: x as uint64 against ora_smoother_pre / post, ora_cf_jacobi and
              ora_cf_twostage; with the residual fused (fuse 1) and with the pending F pass (fuse 2)
              r is uint64-equal to b followed by ora_mv_amxpy(-1) on the new x, the sum of its squares
              uint64-equal to that of the unfused run (the smoother, then a residual SpMV with its
              norm, on the same storage) and within 1e-13 relative of numpy's sum of squares (DESIGN.md
              5); the stall word is zero everywhere;
  switches    one case per format with its switch off: identical results, and the fallback format.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import amg_amd as A
import format_cases as F
import oracle
from amg_amd._native import SSS_SMTR, dptr, iptr
from conftest import vec

pytestmark = pytest.mark.gpu

_mats, _refs = {}, {}


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _mat(c):
    if c.name not in _mats:
        _mats[c.name] = A.NumpyCSR(c.rp, c.ci, c.v, ncols=c.ncols)
    return _mats[c.name]


def _vectors(c):
    """(x, b, y0) of a case: fixed seeds, shared by everything that runs on it"""
    key = (c.name, "vec")
    if key not in _refs:
        rng = np.random.default_rng(sum(map(ord, c.name)))
        _refs[key] = (rng.standard_normal(c.ncols), rng.standard_normal(c.n), rng.standard_normal(c.n))
    return _refs[key]


#: (op, alpha, cap): ACC with its row cap off, below n and above n
def _spmv_ops(n):
    return [("mxy", 1.0, 0), ("amxpy", 0.75, 0), ("resid", -1.0, 0), ("acc", 1.0, n // 3), ("acc", 1.0, n + 7)]


def _spmv_ref(c, op, alpha, cap):
    key = (c.name, op, alpha, cap)
    if key not in _refs:
        ora, M = oracle.load(), _mat(c).mat
        x, b, y0 = _vectors(c)
        y = y0.copy()
        if op == "mxy":
            ora.ora_mv_mxy(C.byref(M), dptr(x), dptr(y))
        elif op == "amxpy":
            ora.ora_mv_amxpy(alpha, C.byref(M), dptr(x), dptr(y), 0)
        elif op == "resid":
            y[:] = b
            ora.ora_mv_amxpy(alpha, C.byref(M), dptr(x), dptr(y), 0)
        else:
            ora.ora_mv_acc(C.byref(M), dptr(x), dptr(y), cap)
        _refs[key] = y
    return _refs[key]


def _check_spmv(c, enc, want, what=""):
    x, b, y0 = _vectors(c)
    for op, alpha, cap in _spmv_ops(c.n):
        y, info = A.spmv_enc(op, alpha, _mat(c).mat, x, b, y0, cap, enc, c.nF)
        assert info == want, (c.name, what, enc, info, want)   # the format first: nothing passes on another one
        ref = _spmv_ref(c, op, alpha, cap)
        assert _bits(y, ref), (c.name, what, enc, op, cap, int(np.count_nonzero(y.view(np.uint64) != ref.view(np.uint64))))
        if op == "acc" and cap < c.n:
            assert _bits(y[cap:], y0[cap:]), (c.name, op, cap)


def _mark(c):
    return np.array([0] * c.nF + [1] * (c.n - c.nF), dtype=np.int32)


def _smooth_ref(c, kind, inner, sweeps, post):
    """(x, r = b - A x) of the oracle's smoother call from the case's (b, x0)"""
    key = (c.name, kind, inner, sweeps, post)
    if key not in _refs:
        ora, M = oracle.load(), _mat(c).mat
        _, b, x0 = _vectors(c)
        x, mark = x0.copy(), _mark(c)
        if kind == "jacobi" and inner > 0:
            ora.ora_cf_twostage(dptr(x), C.byref(M), dptr(b), sweeps, iptr(mark), inner)
        elif kind == "jacobi":
            ora.ora_cf_jacobi(dptr(x), C.byref(M), dptr(b), sweeps, iptr(mark))
        else:
            s = SSS_SMTR()
            s.smoother = 2   # SSS_SM_GS
            s.A, s.b, s.x = C.pointer(M), C.pointer(vec(b)), C.pointer(vec(x))
            s.nsweeps = sweeps
            s.istart, s.iend, s.istep = 0, c.n - 1, -1 if post else 1
            s.cf_order, s.ordering = 1, iptr(mark)
            (ora.ora_smoother_post if post else ora.ora_smoother_pre)(C.byref(s))
        r = b.copy()
        ora.ora_mv_amxpy(-1.0, C.byref(M), dptr(x), dptr(r), 0)
        assert np.isfinite(x).all() and np.isfinite(r).all(), key
        _refs[key] = (x, r)
    return _refs[key]


def _check_level_steps(c, need_pend=False, configs=None):
    """every smoother configuration of a square case through sss_hip_host_level_step; returns the
    results keyed by configuration (test_switch_neutrality compares two such runs)"""
    M, want = _mat(c).mat, c.variants[0][1]
    _, b, x0 = _vectors(c)
    out = {}
    for kind in c.kinds:
        for inner in ((0,) if kind == "exact" else c.inners):
            for sweeps in (1, 2):
                for post in (False, True):
                    cfg = (kind, inner, sweeps, post)
                    if configs is not None and cfg not in configs:
                        continue
                    xr, rr = _smooth_ref(c, kind, inner, sweeps, post)
                    base = None
                    for fuse in (0, 1, 2):
                        where = (c.name,) + cfg + (fuse,)
                        x, r, rn, info, plan = A.level_step(M, c.nF, c.enc, kind, inner, sweeps, post, fuse, b, x0)
                        assert info == want, (where, info, want)
                        assert plan["range_f"] == 1 and plan["range_c"] == 1, (where, plan)   # the range kernels
                        assert plan["inner"] == inner, (where, plan)
                        copies = c.split_copies if inner > 0 else dict.fromkeys(c.split_copies, 0)
                        assert {k: plan[k] for k in copies} == copies, (where, plan, copies)
                        assert plan["stall"] == 0, where
                        exact_bip = kind == "exact"
                        assert plan["fuse_resid"] == int(exact_bip) and plan["f_overwritten"] == int(exact_bip), (where, plan)
                        if need_pend and exact_bip:
                            assert plan["pend_ok"] == 1, (where, plan)   # the MODE 3 pair path must run
                        if fuse == 2 and not plan["pend_ok"]:
                            assert x is None and not exact_bip, where
                            continue
                        assert plan["fused"] == int(fuse > 0 and exact_bip), (where, plan)
                        assert _bits(x, xr), (where, int(np.count_nonzero(x.view(np.uint64) != xr.view(np.uint64))))
                        assert _bits(r, rr), (where, int(np.count_nonzero(r.view(np.uint64) != rr.view(np.uint64))))
                        ref2 = float(np.sum(rr * rr))
                        print(f"{where}: rnorm2 {rn!r} numpy {ref2!r} rel {abs(rn - ref2) / ref2:.2e}")
                        assert abs(rn - ref2) <= 1e-13 * ref2, (where, rn, ref2)
                        if fuse == 0:
                            base = rn
                        else:
                            assert np.float64(rn).view(np.uint64) == np.float64(base).view(np.uint64), (where, rn, base)
                        out[cfg + (fuse,)] = (x, r, rn)
    return out


def _run_case(name):
    c = F.case(name)
    for k, (enc, want) in enumerate(c.variants):
        _check_spmv(c, enc, want, f"variant {k}")
    if c.kinds:
        _check_level_steps(c, need_pend=name.startswith("ell8_pairs"))


@pytest.mark.parametrize("name", F.GROUPS["ell"])
def test_dictionary_ell_limits(name):
    """31 offsets and 8 values in a block with code 0xFE, rows of 8 without a pad and an empty row; one
    offset or value more (not a dictionary ELL, same sums); rows of exactly 16 and 32 and their
    neighbours of 17 and 33; the W = 8 pair kernel over odd class splits, a class of one row and an odd
    block count, exact and Jacobi, with the fused and the pending-F forms; per-row bases."""
    _run_case(name)


@pytest.mark.parametrize("name", F.GROUPS["xell"])
def test_column_ell_limits(name):
    """Every row width with the longest row exactly on it, and one entry more; too sparse to pad; 40
    codes only with ENC_MERGED_ONLY, as a level matrix and as two-stage copies; blocks halved to 16 rows
    of exactly 512 values, and to 12 and 13 rows; 24 column bits with 256 values and the last column
    under the highest value index."""
    _run_case(name)


@pytest.mark.parametrize("name", F.GROUPS["tile"])
def test_tile_limits(name):
    """Dictionary tiles at 256 offsets and 256 values, value-dictionary sorted tiles at 256 values, each
    with one more; a sorted-tile cluster spanning one column less than the diagonal mark, and one
    more (stored-order staging)."""
    _run_case(name)


def test_every_case_ran_or_fails():
    """no case is left out of the three groups above (a case that does not qualify fails, none skips)"""
    assert sorted(sum(F.GROUPS.values(), [])) == sorted(F.NAMES)


# ---------------------------------------------------------------- switch neutrality
def _fallback(c, fmt, blocks, **kw):
    return F.info(fmt, blocks, c.nF, **kw)


def _switch_cases():
    X = F.FMT_DICT | F.FMT_XELL
    c = F.case("ell8_full")
    yield "SSS_HIP_ELL", c, _fallback(c, X, F.xell_choice(c.rp, c.v, c.n, c.nF, c.enc)[2], xell_w=8, shift=23)
    c = F.case("xell_w16")
    yield "SSS_HIP_XELL", c, _fallback(c, F.FMT_DICT, F.tile_blocks(c.rp, c.nF))
    c = F.case("ell_based_R")
    yield "SSS_HIP_ELL_BASE", c, _fallback(c, X, F.row_chunks(c.n), xell_w=8, shift=23)
    c = F.case("dtile_full")
    yield "SSS_HIP_DICT", c, _fallback(c, F.FMT_SORTED, F.tile_blocks(c.rp, c.nF))
    c = F.case("sorted_span")
    yield "SSS_HIP_SORTED_TILES", c, _fallback(c, 0, F.tile_blocks(c.rp))


@pytest.mark.parametrize("switch", ["SSS_HIP_ELL", "SSS_HIP_XELL", "SSS_HIP_ELL_BASE", "SSS_HIP_DICT", "SSS_HIP_SORTED_TILES"])
def test_switch_neutrality(switch, monkeypatch):
    """One case per format with that format's switch at 0: the store info shows the fallback, the four
    SpMV ops and (square cases) the Jacobi level steps give the same uint64 as with the format."""
    _, c, fallback = next(t for t in _switch_cases() if t[0] == switch)
    assert fallback != c.variants[0][1]
    configs = [("jacobi", 0, 2, False), ("jacobi", 1, 1, True)]
    monkeypatch.delenv(switch, raising=False)
    _check_spmv(c, c.enc, c.variants[0][1], "switch on")
    on = _check_level_steps(c, configs=configs) if c.kinds else {}
    monkeypatch.setenv(switch, "0")
    _check_spmv(c, c.enc, fallback, "switch off")   # against the same oracle results
    if c.kinds:
        M = _mat(c).mat
        _, b, x0 = _vectors(c)
        for (kind, inner, sweeps, post, fuse), (x1, r1, n1) in on.items():
            x, r, rn, info, plan = A.level_step(M, c.nF, c.enc, kind, inner, sweeps, post, fuse, b, x0)
            assert info == fallback, (switch, info, fallback)
            assert plan["stall"] == 0 and plan["range_f"] == 1 and plan["range_c"] == 1, plan
            assert _bits(x, x1) and _bits(r, r1), (switch, kind, inner, sweeps, post, fuse)
            assert np.float64(rn).view(np.uint64) == np.float64(n1).view(np.uint64), (switch, rn, n1)
