#!/usr/bin/env python
"""Measurements for DESIGN.md §6.3 (AMG-preconditioned flexible GMRES), one process, one GPU:

- iterations and time to solution of fgmres, pcg and the V-cycle loop on the 7-point n^3 problem
  (hybrid smoother, direct coarse solve, b = 1, x0 = 0), each run once to warm up (graph capture,
  workspace allocation) and then timed: a host clock around calls that end in a stream synchronise;
- the time of one fused orthogonalisation step at j = 5, 10, 20 against the same step as a chain of
  launch_dot + launch_axpy_ratio (sss_lab_time_orth: device events, the two alternating rep by rep).

Writes one JSON document to --out and prints it.  Needs a GPU; there is no fallback.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import amg_amd as A  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--restart", type=int, default=20)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--maxit", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if A.device_count() < 1:
        print("no HIP device visible", file=sys.stderr)
        return 1
    lib = A.lib()
    lib.sss_lab_time_orth.restype = C.c_int
    lib.sss_lab_time_orth.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    res = {"problem": f"7-pt {args.n}^3", "mode": "hybrid/direct", "restart": args.restart, "tol": args.tol}
    n = args.n ** 3

    orth = []
    for j in (5, 10, 20):
        f, c = C.c_double(), C.c_double()
        rc = lib.sss_lab_time_orth(n, j, args.reps, C.byref(f), C.byref(c))
        if rc != 0:
            print(f"sss_lab_time_orth failed ({rc})", file=sys.stderr)
            return 1
        k = j + 1
        orth.append({"j": j, "fused_ms": f.value, "chain_ms": c.value, "fused_over_chain": f.value / c.value,
                     "fused_model_bytes": (4 * k + 6) * 8 * n, "chain_model_bytes": 5 * k * 8 * n,
                     "fused_GBps": (4 * k + 6) * 8 * n / f.value / 1e6, "chain_GBps": 5 * k * 8 * n / c.value / 1e6})
        print(f"[orth] {orth[-1]}", file=sys.stderr, flush=True)
    res["orth_step"] = orth

    t0 = time.perf_counter()
    M = A.generate(7, args.n)   # stays alive: level 0 of the hierarchy is this operator
    D = A.DeviceHierarchy(None, setup_from=M, smoother="hybrid", coarse="direct")
    res["setup_s"] = time.perf_counter() - t0
    b, x0 = np.ones(n), np.zeros(n)
    nb = float(np.sqrt(n))

    def vcycle():
        rel = []
        while len(rel) < args.maxit:
            D.cycle()
            rel.append(D.residual_norm() / nb)
            if rel[-1] < args.tol:
                break
        return len(rel), rel

    solvers = {"vcycle": vcycle, "pcg": lambda: D.pcg(args.tol, args.maxit),
               "fgmres": lambda: D.fgmres(args.tol, args.restart, args.maxit)}
    res["solves"] = {}
    for name, fn in solvers.items():
        runs = []
        for rep in range(3):   # the first warms up
            D.upload(0, "b", b)
            D.upload(0, "x", x0)
            D.sync()
            t0 = time.perf_counter()
            its, hist = fn()
            D.sync()
            dt = time.perf_counter() - t0
            true_rel = D.residual_norm() / nb
            runs.append({"iterations": int(its), "seconds": dt, "last_estimate": float(hist[-1]), "true_relres": true_rel})
        res["solves"][name] = {"warmup": runs[0], "timed": runs[1:]}
        print(f"[solve] {name}: {runs}", file=sys.stderr, flush=True)
    D.close()
    text = json.dumps(res, indent=1)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
