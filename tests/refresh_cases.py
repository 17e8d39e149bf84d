"""Shared by the refresh tests (tests/test_refresh_cpu.py, tests/test_gpu_refresh.py): the matrices, the
drift rule that gives "new values on the same pattern", hierarchy digests and the comparison helpers."""
from __future__ import annotations

import ctypes as C
import hashlib

import numpy as np

import amg_amd as A
from amg_amd import workloads as W
from conftest import BUS_MTX, quiet_ctx

#: (amp, shift) of the convergence table in DESIGN.md 6.6
DRIFTS = [(0.0, 0.25), (0.3, 0.0), (0.6, 0.0), (0.9, 0.1)]
CPU_MATRICES = ["p7_12", "p7_16", "a27_8", "bus", "circuit3000"]

_keep = {}


def matrix(name: str) -> A.SSS_MAT:
    """The named operator (generated or read once per process; the SSS_MAT is shared: do not write to it)."""
    if name not in _keep:
        if name == "bus":
            _keep[name] = (A.read_mtx(BUS_MTX), None)
        elif name.startswith("circuit"):
            k = W.circuit_csr(int(name[len("circuit"):]))
            _keep[name] = (k.mat, k)
        else:
            kind, n = name.split("_")
            _keep[name] = (A.generate({"p7": 7, "a27": 27}[kind], int(n)), None)
    return _keep[name][0]


def drift_values(rp, ci, v, amp: float, shift: float) -> np.ndarray:
    """New values on the pattern (rp, ci): every off-diagonal entry scaled by 1 + amp * (2 u - 1) with u in
    [0, 1) a hash of the unordered index pair (so a symmetric operator stays symmetric), the diagonal
    set so that the row keeps its sum (constants stay near-null), plus shift * |old diagonal|."""
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    lo, hi = np.minimum(rows, ci).astype(np.uint64), np.maximum(rows, ci).astype(np.uint64)
    h = (lo * np.uint64(0x9E3779B97F4A7C15) ^ (hi + np.uint64(12345)) * np.uint64(0xC2B2AE3D27D4EB4F)) >> np.uint64(11)
    u = h.astype(np.float64) / float(1 << 53); off = rows != ci
    v2 = v.copy(); v2[off] = v[off] * (1.0 + amp * (2 * u[off] - 1))
    excess = np.bincount(rows, weights=v, minlength=n); offsum = np.bincount(rows[off], weights=v2[off], minlength=n)
    d = np.flatnonzero(~off); v2[d] = excess[rows[d]] - offsum[rows[d]] + shift * np.abs(v[d])
    return v2


def drifted(M: A.SSS_MAT, amp: float, shift: float) -> A.NumpyCSR:
    rp, ci, v = A.csr_arrays(M)
    with np.errstate(over="ignore"):   # the hash multiplies modulo 2^64
        return A.NumpyCSR(rp, ci, drift_values(rp, ci, v, amp, shift), ncols=M.num_cols)


def scaled(M: A.SSS_MAT, f: float) -> A.NumpyCSR:
    rp, ci, v = A.csr_arrays(M)
    return A.NumpyCSR(rp, ci, v * f, ncols=M.num_cols)


def hierarchy(M: A.SSS_MAT) -> A.Hierarchy:
    with quiet_ctx():
        return A.Hierarchy(M)


def cfmark(H, l) -> np.ndarray:
    L = H.level(l)
    return np.ctypeslib.as_array(L.cfmark.d, shape=(L.A.num_rows,)).copy()


def digest(H, transfer: bool = True) -> str:
    """sha256 over A of every level and (transfer) P, R, cfmark of every level but the coarsest, as bytes."""
    h = hashlib.sha256()
    h.update(bytes([H.num_levels]))
    for l in range(H.num_levels):
        mats = [H.level(l).A] + ([H.level(l).P, H.level(l).R] if transfer and l + 1 < H.num_levels else [])
        for M in mats:
            h.update(np.array([M.num_rows, M.num_cols, M.num_nnzs], np.int64).tobytes())
            for arr in A.csr_arrays(M):
                h.update(arr.tobytes())
        if transfer and l + 1 < H.num_levels:
            h.update(cfmark(H, l).tobytes())
    return h.hexdigest()


def same_bits(M1, M2) -> bool:
    a, b = A.csr_arrays(M1), A.csr_arrays(M2)
    return (M1.num_rows, M1.num_cols, M1.num_nnzs) == (M2.num_rows, M2.num_cols, M2.num_nnzs) and all(
        np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def pattern_copy(Cm: A.SSS_MAT, fill: float = np.nan) -> A.NumpyCSR:
    """C's pattern with every value set to `fill` (what a values-only product must overwrite)."""
    rp, ci, v = A.csr_arrays(Cm)
    return A.NumpyCSR(rp, ci, np.full(len(v), fill), ncols=Cm.num_cols)


def signed_zero_case():
    """3 x 3: R = P = I, A = [[-0.0, -0.0, 1], [2, 3, 0], [0, 4, 5]] stored diagonal first.  Row 0 of
    R A P: the diagonal's only product is 1 * -0.0 * 1 = -0.0, added to the 0.0 it starts from: +0.0;
    column 1's only product is -0.0, assigned: -0.0 (a slot started at +0.0 would give +0.0)."""
    eye = lambda: A.NumpyCSR([0, 1, 2, 3], [0, 1, 2], [1.0, 1.0, 1.0])  # noqa: E731
    Am = A.NumpyCSR([0, 3, 5, 7], [0, 1, 2, 1, 0, 2, 1], [-0.0, -0.0, 1.0, 3.0, 2.0, 5.0, 4.0])
    return eye(), Am, eye()


def host_rap(R, Am, P) -> A.SSS_MAT:
    """SSS_blas_mat_rap (the caller destroys it)."""
    return A.lib().SSS_blas_mat_rap(C.byref(R), C.byref(Am), C.byref(P))
