#!/usr/bin/env python
"""Measurements for DESIGN.md 6.6 (refresh of a set-up hierarchy for new operator values), one
process, one GPU, 7-point n^3 in throughput mode (hybrid smoother, direct coarse solve):

  - the old hierarchy is set up on the operator M (sss_hip_setup_create); the new operator N is M
    under the drift rule of tests/refresh_cases.py with (amp, shift) = (0.3, 0);
  - alternated, --samples times each: a fresh sss_hip_setup_create on N (setup and mirror seconds),
    and SSS_amg_refresh + sss_hip_hier_refresh of the old hierarchy to N (chain and mirror seconds,
    with the [refresh] line of every level, the library's stderr kept verbatim);
  - warmed-up V-cycle and PCG iterations to --tol with their wall times on the fresh and on the
    refreshed hierarchy (b = standard_normal, seed 1, x0 = 0);
  - hbm_used_bytes() before the first refresh and after the last one;
  - per level of the refreshed hierarchy: sss_hip_rap against sss_hip_rap_values (each forced, wall
    seconds with copies and kernels apart) and SSS_blas_mat_rap against sss_rap_values_host, all four
    checked to agree on bits.

Writes one JSON document to --out and prints it.  Needs a GPU; there is no fallback.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import amg_amd as A  # noqa: E402


class capture_fds:
    """The C library's stdout and stderr of a block, as text (fd level)."""

    def __enter__(self):
        sys.stdout.flush()
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = [os.dup(1), os.dup(2)]
        os.dup2(self.tmp.fileno(), 1)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        C.CDLL(None).fflush(None)
        os.dup2(self.saved[0], 1)
        os.dup2(self.saved[1], 2)
        for fd in self.saved:
            os.close(fd)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def drift_values(rp, ci, v, amp: float, shift: float) -> np.ndarray:
    """The drift rule of tests/refresh_cases.py (row sums kept, symmetric in the index pair)."""
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    lo, hi = np.minimum(rows, ci).astype(np.uint64), np.maximum(rows, ci).astype(np.uint64)
    h = (lo * np.uint64(0x9E3779B97F4A7C15) ^ (hi + np.uint64(12345)) * np.uint64(0xC2B2AE3D27D4EB4F)) >> np.uint64(11)
    u = h.astype(np.float64) / float(1 << 53)
    off = rows != ci
    v2 = v.copy()
    v2[off] = v[off] * (1.0 + amp * (2 * u[off] - 1))
    excess = np.bincount(rows, weights=v, minlength=n)
    offsum = np.bincount(rows[off], weights=v2[off], minlength=n)
    d = np.flatnonzero(~off)
    v2[d] = excess[rows[d]] - offsum[rows[d]] + shift * np.abs(v[d])
    return v2


def solves(D, b, nb, tol, maxit) -> dict:
    """V-cycle loop and PCG to tol: the first run warms up (graph capture), the second is timed."""
    x0 = np.zeros(len(b))

    def vcycle():
        rel = []
        while len(rel) < maxit:
            D.cycle()
            rel.append(D.residual_norm() / nb)
            if rel[-1] < tol:
                break
        return len(rel), rel

    out = {}
    for solver, fn in (("vcycle", vcycle), ("pcg", lambda: D.pcg(tol, maxit))):
        for _ in range(2):
            D.upload(0, "b", b)
            D.upload(0, "x", x0)
            D.sync()
            t0 = time.perf_counter()
            its, hist = fn()
            D.sync()
            dt = time.perf_counter() - t0
            out[solver] = {"iterations": int(its), "seconds": dt, "last_relres": float(hist[-1]),
                           "true_relres": D.residual_norm() / nb}
    return out


def same_bits(M1, M2) -> bool:
    a, b = A.csr_arrays(M1, copy=False), A.csr_arrays(M2, copy=False)
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def chain_detail(H) -> list:
    lib = A.lib()
    times = (C.c_double * 2)()
    rows = []
    for l in range(H.num_levels - 1):
        L, Cl = H.level(l), H.level(l + 1).A
        r = {"level": l, "rows_A": L.A.num_rows, "nnz_A": L.A.num_nnzs, "rows_C": Cl.num_rows, "nnz_C": Cl.num_nnzs}
        Cg = A.SSS_MAT()
        t0 = time.perf_counter()
        rc = lib.sss_hip_rap(C.byref(L.R), C.byref(L.A), C.byref(L.P), C.byref(Cg))
        r["device_rap_s"] = time.perf_counter() - t0
        assert rc == 0, rc
        lib.sss_hip_rap_times(times)
        r["device_rap_copies_s"], r["device_rap_kernels_s"] = times[0], times[1]
        assert same_bits(Cg, Cl), l
        # the values-only products write the values the refreshed level already holds
        lib.SSS_blas_array_set(Cg.num_nnzs, Cg.val, C.c_double(np.nan))
        t0 = time.perf_counter()
        rc = lib.sss_hip_rap_values(C.byref(L.R), C.byref(L.A), C.byref(L.P), C.byref(Cg))
        r["device_values_s"] = time.perf_counter() - t0
        assert rc == 0, rc
        lib.sss_hip_rap_times(times)
        r["device_values_copies_s"], r["device_values_kernels_s"] = times[0], times[1]
        assert same_bits(Cg, Cl), l
        lib.SSS_blas_array_set(Cg.num_nnzs, Cg.val, C.c_double(np.nan))
        t0 = time.perf_counter()
        rc = lib.sss_rap_values_host(C.byref(L.R), C.byref(L.A), C.byref(L.P), C.byref(Cg))
        r["host_values_s"] = time.perf_counter() - t0
        assert rc == 0 and same_bits(Cg, Cl), l
        lib.SSS_mat_destroy(C.byref(Cg))
        t0 = time.perf_counter()
        Ch = lib.SSS_blas_mat_rap(C.byref(L.R), C.byref(L.A), C.byref(L.P))
        r["host_rap_s"] = time.perf_counter() - t0
        assert same_bits(Ch, Cl), l
        lib.SSS_mat_destroy(C.byref(Ch))
        rows.append(r)
        print(f"[chain] {r}", file=sys.stderr, flush=True)
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--maxit", type=int, default=100)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--amp", type=float, default=0.3)
    ap.add_argument("--shift", type=float, default=0.0)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if A.device_count() < 1:
        print("no HIP device visible", file=sys.stderr)
        return 1
    os.environ["SSS_SETUP_TIMING"] = "1"
    lib = A.lib()
    lib.sss_hip_rap_times.restype, lib.sss_hip_rap_times.argtypes = None, [C.POINTER(C.c_double)]
    lib.SSS_blas_array_set.restype, lib.SSS_blas_array_set.argtypes = None, [C.c_int, C.POINTER(C.c_double), C.c_double]
    n = args.n ** 3
    mode = dict(smoother="hybrid", coarse="direct")
    res = {"problem": f"7-pt {args.n}^3", "rows": n, "mode": "hybrid/direct", "tol": args.tol,
           "drift": [args.amp, args.shift], "fresh": [], "refresh": []}
    M = A.generate(7, args.n)
    rp, ci, v = A.csr_arrays(M, copy=False)
    N = A.NumpyCSR(rp, ci, drift_values(rp, ci, v, args.amp, args.shift))
    b = np.random.default_rng(1).standard_normal(n)
    nb = float(np.linalg.norm(b))

    with capture_fds():
        D = A.DeviceHierarchy(None, setup_from=M, **mode)
    res["old_setup"] = {"setup_s": D.times[0], "mirror_after_s": D.times[1], "levels": D.H.num_levels,
                        "rows": [D.level_info(l).rows for l in range(D.H.num_levels)],
                        "nnz": [D.level_info(l).nnz for l in range(D.H.num_levels)]}
    res["hbm_used_before_refresh"] = A.hbm_used_bytes()
    for s in range(args.samples):
        t0 = time.perf_counter()
        with capture_fds() as cap:
            F = A.DeviceHierarchy(None, setup_from=N.mat, **mode)
        f = {"setup_s": F.times[0], "mirror_after_s": F.times[1], "wall_s": time.perf_counter() - t0,
             "levels": F.H.num_levels}
        if s == 0:
            f["phase_lines"] = [ln for ln in cap.text.splitlines() if ln.startswith("[setup]")]
            res["fresh_solves"] = solves(F, b, nb, args.tol, args.maxit)
        f["hbm_used_with_old_mirror"] = A.hbm_used_bytes()
        F.close()
        F.H.close()
        res["fresh"].append(f)
        print(f"[fresh] {f['setup_s']:.2f} + {f['mirror_after_s']:.2f} s", file=sys.stderr, flush=True)
        with capture_fds() as cap:
            t0 = time.perf_counter()
            D.H.refresh(N.mat)
            t1 = time.perf_counter()
            D.refresh()
            t2 = time.perf_counter()
        r = {"chain_s": t1 - t0, "mirror_s": t2 - t1, "total_s": t2 - t0,
             "level_lines": [ln for ln in cap.text.splitlines() if ln.startswith("[refresh]")],
             "hbm_used_after": A.hbm_used_bytes()}
        res["refresh"].append(r)
        print(f"[refresh] chain {r['chain_s']:.2f} s + mirror {r['mirror_s']:.2f} s", file=sys.stderr, flush=True)
    res["hbm_used_after_last_refresh"] = A.hbm_used_bytes()
    res["refreshed_solves"] = solves(D, b, nb, args.tol, args.maxit)
    res["chain_per_level"] = chain_detail(D.H)
    D.close()
    D.H.close()

    text = json.dumps(res, indent=1)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
