"""GPU tests of the narrow keys of the merged-group kernels (SSS_HIP_MERGE_KEY16, DevCSR::mg_k16).

With narrow keys a merged entry is a 16-bit key (column delta << 3 | accumulator) plus its value; a
descriptor per chunk of 64 entries of a wave's share holds one or two column bases, and a share with
a chunk that fits neither keeps 32-bit keys (tests/test_merged_key16_host.py has the format).  No
entry moves to another lane or accumulator, so every sum must keep its bits: the checks here compare
SSS_HIP_MERGE_KEY16 = 0 and 1, each with both accumulator forms (SSS_HIP_MERGE_ACC), as uint64, for
G in {4, 8} and W in {1, 2, 4}.

The matrix (level 0 of a hierarchy, in the manner of test_gpu_merged_batches.py): rows [0, N0) are a
1-D chain of strong couplings, which the coarsening splits into F (even) and C (odd) rows, each
with one positive (never strong) entry to the same-class row below it; the few hundred rows
[N0, n) have no strong coupling, become F rows, and hold positive entries in clusters of the
relabeled column range (F rows first, then C): near its start, around a third and two thirds of
the F range, and at both ends of the C range (some groups of rows only near the start and at the far
end).  With ~70,000 rows the clusters lie more than 2^13 and -- F against C -- more than 2^16 columns
apart.  A chunk inside one cluster has one base, a chunk across one gap
two, and a chunk that holds a whole small middle cluster with entries of both its neighbours has two
wide gaps and escapes.  Every test first asserts through sss_hip_merged_key_stats that the
[N | L] copy and the L copy of the F class and the level matrix each hold all three; it fails, never
skips, if one does not.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import amg_amd as A
import oracle
from amg_amd._native import dptr
from conftest import build_hierarchy

pytestmark = pytest.mark.gpu

GS = (4, 8)
WS = (1, 2, 4)
N0 = 69000           # chain rows
NT = 360             # cluster rows


def _cluster_rows():
    """per cluster row: its columns (original numbering), all of them F chain rows below it (the L
    segment) or C chain rows (N)"""
    rows = []
    for t in range(NT):
        a, m1, m2, c = 3 + 7 * (t % 23), 1 + t % 5, 1 + (t // 5) % 4, (t % 3) * (4 + 5 * (t % 11))
        f = lambda j: 2 * j            # F chain row with relabeled index j
        cc = lambda j: 2 * j + 1       # C chain row with relabeled index nF + j
        cols = [f(40 + (3 * t) % 50 + 2 * k) for k in range(a)]
        if (t // 16) % 4 != 3:   # (else: the first and the last cluster only, one gap beyond 2^16)
            cols += [f(11500 + (t % 7) + 3 * k) for k in range(m1)]
            cols += [f(23000 + (t % 5) + 2 * k) for k in range(m2 + 9 * (t % 2))]
            cols += [cc(300 + 5 * (t % 13) + 2 * k) for k in range(c)]
        cols += [cc(33000 + (t % 17) + k) for k in range(2 + t % 3)]
        rows.append(sorted(set(cols)))
    return rows


@pytest.fixture(scope="module")
def wide_matrix():
    n = N0 + NT
    rp, ci, v = [0], [], []
    cl = _cluster_rows()
    for i in range(n):
        if i < N0:
            row = {c: -1.0 for c in (i - 1, i + 1) if 0 <= c < N0}
            if i >= 2:
                row[i - 2] = 0.02 + 0.001 * (i % 97)
        else:
            row = {c: 0.02 + 0.001 * ((5 * i + 11 * t) % 160) for t, c in enumerate(cl[i - N0])}
        row[i] = 1.0 + sum(abs(x) for x in row.values())
        for c in sorted(row):
            ci.append(c)
            v.append(row[c])
        rp.append(len(ci))
    return A.NumpyCSR(rp, ci, v)


@pytest.fixture(scope="module")
def wide_h(wide_matrix, quiet):
    H = build_hierarchy(wide_matrix.mat, quiet)
    L = H.level(0)
    n = L.A.num_rows
    mark = np.ctypeslib.as_array(L.cfmark.d, shape=(n,))
    is_c = mark == 1
    assert not is_c[0:N0:2].any() and is_c[1:N0:2].all() and not is_c[N0:].any(), "the C/F split is not the designed one"
    return H


@pytest.fixture(params=[(g, w) for g in GS for w in WS], ids=lambda p: f"G{p[0]}W{p[1]}")
def merged(request, monkeypatch):
    g, w = request.param
    monkeypatch.setenv("SSS_HIP_WAVE_MIN", "1")
    monkeypatch.setenv("SSS_HIP_FREE_MIN", "1")
    monkeypatch.setenv("SSS_HIP_MERGE_MIN_ROWS", "1")
    monkeypatch.setenv("SSS_HIP_MERGE_G", str(g))
    monkeypatch.setenv("SSS_HIP_MERGE_W", str(w))
    return g, w


def _stats(D, level, which):
    out = (C.c_longlong * 8)()
    rc = A.lib().sss_hip_merged_key_stats(D.h, level, which, out)
    assert rc in (0, 1), rc
    return None if rc else dict(zip(("chunks", "one", "two", "wide", "escaped", "nnz", "slots", "esc_keys"), out))


def _arrays(D, level, which):
    s = _stats(D, level, which)
    k16 = np.zeros(max(s["nnz"], 1), np.uint16)
    desc = np.zeros((s["slots"], 4), np.int32)
    esc = np.zeros(max(s["esc_keys"], 1), np.uint32)
    assert A.lib().sss_hip_merged_keys_get(D.h, level, which, k16.ctypes.data, desc.ctypes.data, esc.ctypes.data) == 0
    return s, k16[: s["nnz"]], desc, esc[: s["esc_keys"]]


def _assert_kinds(D, copies=(0, 1, 3)):
    """one-base, two-base and escaped chunks in the level matrix, the F class's [N | L] copy and its L copy"""
    for which in copies:
        s = _stats(D, 0, which)
        assert s is not None, which
        print(f"copy {which}: {s}")
        assert s["one"] > 0 and s["two"] > 0 and s["wide"] > 0 and s["escaped"] >= s["wide"], (which, s)
        assert s["one"] + s["two"] + s["wide"] == s["chunks"] and s["esc_keys"] > 0


def _variants(monkeypatch, run):
    """run() with 32-bit and narrow keys, each with the register and the LDS accumulators"""
    out = {}
    for k16 in ("0", "1"):
        for acc in ("0", "1"):
            monkeypatch.setenv("SSS_HIP_MERGE_KEY16", k16)
            monkeypatch.setenv("SSS_HIP_MERGE_ACC", acc)
            out[k16, acc] = run(k16 == "1")
    return out


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64),
                          np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def _smooth0(H, inner, data, narrow):
    """(b, x0, x) of one pre and one post smoother call on level 0"""
    D = A.DeviceHierarchy(H, smoother="jacobi", coarse="krylov", relabel=1, inner=inner, inner_from=0, sum_order=1)
    out = []
    try:
        assert D.level_info(0).a_format & 8   # merged copies
        if narrow:
            _assert_kinds(D, (0, 1, 3) if inner else (0,))   # (plain C/F-Jacobi has no split copies)
        else:
            assert _stats(D, 0, 0) is None
        n = H.level(0).A.num_rows
        for post in (False, True):
            b, x0 = data(n)
            D.upload(0, "b", b)
            D.upload(0, "x", x0)
            D.smooth(0, post)
            out.append((b, x0, D.download(0, "x")))
    finally:
        D.close()
    return out


def test_spans_and_builders(wide_h, monkeypatch, merged):
    """The copies hold every chunk kind, with bases beyond 2^13 and 2^16 apart; the host-built and
    the device-built arrays are byte-identical; the ledger counts the narrow bytes."""
    H = wide_h
    kw = dict(smoother="jacobi", coarse="krylov", relabel=1, inner=1, inner_from=0, sum_order=1)
    monkeypatch.setenv("SSS_HIP_MERGE_KEY16", "0")
    D = A.DeviceHierarchy(H, **kw)
    try:
        stored32 = D.level_info(0).a_stream_bytes
    finally:
        D.close()
    monkeypatch.setenv("SSS_HIP_MERGE_KEY16", "1")
    got = {}
    for build in ("0", "1"):
        monkeypatch.setenv("SSS_HIP_GPU_BUILD", build)
        D = A.DeviceHierarchy(H, **kw)
        try:
            _assert_kinds(D)
            got[build] = [_arrays(D, 0, which) if _stats(D, 0, which) else None for which in range(5)]
            stored = D.level_info(0).a_stream_bytes
        finally:
            D.close()
        s = got[build][0][0]   # 2 B keys instead of 4 B, the descriptors, the escaped keys
        assert stored == stored32 - 2 * s["nnz"] + 16 * s["slots"] + 4 * s["esc_keys"]
    for which, (h, d) in enumerate(zip(got["0"], got["1"])):
        assert (h is None) == (d is None), which
        if h is None:
            continue
        assert h[0] == d[0], which
        for a, b in zip(h[1:], d[1:]):
            assert a.tobytes() == b.tobytes(), which
    s, k16, desc, esc = got["1"][1]   # the F class's [N | L] copy: F-range against C-range columns
    two = desc[(desc[:, 2] > 0) & (desc[:, 2] < 64) & (desc[:, 3] < 0)]
    jump = two[:, 1] - two[:, 0]
    assert (jump > 1 << 13).any() and (jump > 1 << 16).any()


@pytest.mark.parametrize("inner", [1, 0])
def test_smoother_same_bits(wide_h, monkeypatch, merged, inner):
    """ts_stage0 + ts_inner (inner = 1) and the C/F-Jacobi passes (inner = 0) on level 0."""
    H = wide_h

    def run(narrow):
        rng = np.random.default_rng(51)
        return _smooth0(H, inner, lambda n: (rng.standard_normal(n), rng.standard_normal(n)), narrow)

    out = _variants(monkeypatch, run)
    ref = out["0", "0"]
    for key, res in out.items():
        for k, ((_, _, xr), (_, _, x)) in enumerate(zip(ref, res)):
            assert np.isfinite(x).all() and np.any(x != 0.0)
            assert _same_bits(xr, x), (key, "post" if k else "pre")
    ora = oracle.load()
    L = H.level(0)
    for k, (b, x0, x) in enumerate(out["1", "1"]):
        xo = x0.copy()
        sweeps = H.pars.post_iter if k else H.pars.pre_iter
        if inner > 0:
            ora.ora_cf_twostage(dptr(xo), C.byref(L.A), dptr(b), sweeps, L.cfmark.d, inner)
        else:
            ora.ora_cf_jacobi(dptr(xo), C.byref(L.A), dptr(b), sweeps, L.cfmark.d)
        err = np.linalg.norm(x - xo) / np.linalg.norm(xo)
        print(f"inner {inner} {'post' if k else 'pre'}: relative distance to the oracle {err:.3e}")
        assert err <= 1e-12, (k, err)   # the free-order bound of test_gpu_merged_batches.py


def test_cycles_same_bits(wide_h, monkeypatch, merged):
    """Whole cycles with the residual norm: spmv_merged on the level matrix and the transfers."""
    H = wide_h
    n = H.level(0).A.num_rows

    def run(narrow):
        D = A.DeviceHierarchy(H, smoother="hybrid", coarse="krylov", sum_order=1)
        try:
            assert D.level_info(0).a_format & 8
            if narrow:
                _assert_kinds(D, (0,))
            else:
                assert _stats(D, 0, 0) is None
            D.upload(0, "b", np.ones(n))
            D.upload(0, "x", np.ones(n))
            for _ in range(2):
                D.cycle()
            return D.download(0, "x"), D.residual_norm()
        finally:
            D.close()

    out = _variants(monkeypatch, run)
    x0, r0 = out["0", "0"]
    assert np.isfinite(r0) and r0 > 0.0
    for key, (x, r) in out.items():
        assert _same_bits(x0, x), key
        assert _same_bits([r0], [r]), key


@pytest.fixture(scope="module")
def spmv_matrix():
    """A square matrix without diagonal: short rows but for every 150th, which holds the cluster
    rows' columns spread over the whole column range"""
    n = 70001
    cl = _cluster_rows()
    rp, ci, v = [0], [], []
    for q in range(n):
        cols = [c for c in (q - 1, q - 3) if c >= 0]
        if q % 150 == 149 and q // 150 < NT:
            src = cl[q // 150]
            cols = sorted({(c // 2 + (35000 if c % 2 else 0)) for c in src} | set(cols))
        for c in sorted(cols):
            ci.append(c)
            v.append((-1.0) ** c * (0.25 + 0.001 * ((7 * q + 3 * c) % 500)))
        rp.append(len(ci))
    return A.NumpyCSR(rp, ci, v), n


def _stored_order_counts(M, n, g, w):
    """chunk kinds of the merged copy of M's rows in stored order, through the host narrowing"""
    rp = np.asarray(M.rp[: n + 1], dtype=np.int64)
    ci = np.asarray(M.ci[: rp[-1]], dtype=np.int64)
    row = np.repeat(np.arange(n), np.diff(rp))
    key = (row // g) << 32 | ci << 4 | row % g
    keys = (np.sort(key) & 0xFFFFFFFF).astype(np.uint32)
    ng = (n + g - 1) // g
    gp = rp[np.minimum(np.arange(ng + 1) * g, n)].astype(np.int32)
    cap = (keys.size >> 6) + ng * w + 1
    k16, desc, esc = np.zeros(keys.size, np.uint16), np.zeros((cap, 4), np.int32), np.zeros(keys.size, np.uint32)
    nd, ne, cnt = C.c_longlong(), C.c_longlong(), (C.c_longlong * 5)()
    assert A.lib().sss_hip_merged_narrow(keys.ctypes.data, keys.size, gp.ctypes.data_as(C.POINTER(C.c_int)), ng, 0, w,
                                         k16.ctypes.data, desc.ctypes.data, cap, C.byref(nd), esc.ctypes.data, esc.size,
                                         C.byref(ne), cnt) == 0
    return list(cnt)


def test_spmv_ops_same_bits(spmv_matrix, monkeypatch, merged):
    """The four SpMV ops of spmv_merged (sss_hip_host_spmv_order, free order)."""
    M, n = spmv_matrix
    g, w = merged
    cnt = _stored_order_counts(M, n, g, w)
    print(f"chunks {cnt}")
    assert cnt[1] > 0 and cnt[2] > 0 and cnt[3] > 0 and cnt[4] >= cnt[3], cnt
    lib = A.lib()
    ora = oracle.load()
    rng = np.random.default_rng(54)
    for op in ("mxy", "amxpy", "resid", "acc"):
        x, b, y0 = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
        alpha = -1.0 if op in ("resid", "amxpy") else 1.0
        cap = 1000 if op == "acc" else 0

        def run(narrow):
            y = y0.copy()
            assert lib.sss_hip_host_spmv_order(A.SPMV[op], alpha, C.byref(M.mat), dptr(x), dptr(b), dptr(y), cap, 1) == 0
            return y

        out = _variants(monkeypatch, run)
        for key, y in out.items():
            assert _same_bits(out["0", "0"], y), (op, key)
        y = out["1", "1"]
        y_ref = y0.copy()
        if op == "mxy":
            ora.ora_mv_mxy(C.byref(M.mat), dptr(x), dptr(y_ref))
        elif op == "amxpy":
            ora.ora_mv_amxpy(alpha, C.byref(M.mat), dptr(x), dptr(y_ref), 0)
        elif op == "resid":
            y_ref[:] = b
            ora.ora_mv_amxpy(-1.0, C.byref(M.mat), dptr(x), dptr(y_ref), 0)
        else:
            ora.ora_mv_acc(C.byref(M.mat), dptr(x), dptr(y_ref), cap)
        assert not _same_bits(y, y0)
        err = np.linalg.norm(y - y_ref) / np.linalg.norm(y_ref)
        print(f"{op}: relative distance to the oracle {err:.3e}")
        assert err <= 1e-12, (op, err)
    lib.sss_hip_host_cache_clear()


def test_subnormal_and_signed_zero(wide_h, monkeypatch, merged):
    """b and x0 scaled by 2^-1040: every product and partial sum is subnormal; then x0 = 0 with
    -0.0 entries in b: every product is a signed zero (the cases of test_gpu_merged_acc.py)."""
    H = wide_h
    scale = 2.0 ** -1040

    def tiny(narrow):
        rng = np.random.default_rng(52)
        return _smooth0(H, 1, lambda n: (scale * rng.standard_normal(n), scale * rng.standard_normal(n)), narrow)

    def zeros(narrow):
        rng = np.random.default_rng(53)

        def data(n):
            b = rng.standard_normal(n)
            b[rng.random(n) < 0.5] = -0.0
            return b, np.zeros(n)
        return _smooth0(H, 1, data, narrow)

    out = _variants(monkeypatch, tiny)
    for key, res in out.items():
        for (_, _, xr), (_, _, x) in zip(out["0", "0"], res):
            assert np.any(x != 0.0) and np.abs(x).max() < 2.0 ** -1022   # subnormal results, not flushed
            assert _same_bits(xr, x), key
    out = _variants(monkeypatch, zeros)
    for key, res in out.items():
        for (_, _, xr), (_, _, x) in zip(out["0", "0"], res):
            assert _same_bits(xr, x), key
