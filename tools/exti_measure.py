#!/usr/bin/env python
"""Measurements for DESIGN.md 6.7 (the extended+i interpolation, interp_type 3), one process, one GPU,
7-point n^3, PMIS coarsening, interp_type 2 against interp_type 3:

  - per interpolation two host-only setups (SSS_amg_setup) of the same operator, every level's pattern
    and weights forced to the device (SSS_SETUP_GPU_INTERP=1, SSS_SETUP_GPU_INTERP_MIN=0) and to the host
    (SSS_SETUP_GPU_INTERP=0): per level rows, nnz(A), nnz(P), the device weights' seconds with copies and
    kernels split, the host weights' seconds (OpenMP, the threads of this process);
  - per interpolation one setup + mirror (sss_hip_setup_create, throughput mode: hybrid smoother, direct
    coarse solve) at the library's thresholds: setup and mirror seconds, levels, rows per level, operator
    complexity, ms per iteration (time_iterations, the two hierarchies alternated sample by sample),
    V-cycle and PCG iterations to --tol with their wall times (b = standard_normal, seed 1, x0 = 0), and
    setup + mirror + solve: operator to answer; per level the largest |p|, the F rows without a pattern
    and the isolated rows; and the V-cycle loop on the same hierarchy in parity mode (exact GS-CF, Krylov
    coarse solve), at most --parity-cycles cycles.

--pmax N runs everything with the cap on the entries per row of P (SSS_SETUP_PMAX=N) and adds
the truncation's own seconds on either side to the per-level records; --pmax 0 keeps the cap off and reports
the uncapped truncation's seconds the same way.

Writes one JSON document to --out and prints it.  Needs a GPU; there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import amg_amd as A  # noqa: E402
from interp_measure import ENV, environment  # noqa: E402
from pmis_measure import capture_fds, make_pars  # noqa: E402

VARIANTS = {"pmis_interp2": 2, "pmis_interp3": 3}
DEV = re.compile(r"(standard|extended\+i) P: device weights, (\d+) rows, (\d+) entries, (\d+) lanes per row, "
                 r"(\d+) rows on global tables, copies ([0-9.]+) s, kernels ([0-9.]+) s")
HOST = re.compile(r"(standard|extended\+i) P: host weights ([0-9.]+) s, (\d+) rows, (\d+) entries")
# the truncation's own seconds, printed when SSS_SETUP_PMAX is set (--pmax): a note at the end of
# the device line, a line of its own before the host line (row-parallel form only: P of 2^20 entries or more)
DEV_TRUNC = re.compile(r", (?:cap (\d+) at (\d+) lanes per row|no cap), truncation ([0-9.]+) s")
HOST_TRUNC = re.compile(r"truncation: host, cap (\d+), (\d+) rows, (\d+) of (\d+) entries kept, ([0-9.]+) s")


def weight_lines(text: str) -> list:
    """One record per level from the weights' timing lines of one setup."""
    out = []
    host_trunc = None
    for line in text.splitlines():
        m = DEV.search(line)
        if m:
            out.append({"where": "device", "rows": int(m.group(2)), "entries": int(m.group(3)), "lanes": int(m.group(4)),
                        "global_rows": int(m.group(5)), "copies_s": float(m.group(6)), "kernels_s": float(m.group(7)),
                        "seconds": float(m.group(6)) + float(m.group(7))})
            t = DEV_TRUNC.search(line)
            if t:
                out[-1].update(trunc_lanes=int(t.group(2)) if t.group(2) else 1, trunc_s=float(t.group(3)))
        m = HOST_TRUNC.search(line)
        if m:
            host_trunc = {"trunc_s": float(m.group(5)), "trunc_entries_before": int(m.group(4))}
        m = HOST.search(line)
        if m:
            out.append({"where": "host", "rows": int(m.group(3)), "entries": int(m.group(4)), "seconds": float(m.group(2))})
            out[-1].update(host_trunc or {})
            host_trunc = None
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--maxit", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5, help="alternated timing samples per hierarchy (at least 3)")
    ap.add_argument("--iters", type=int, default=10, help="iterations per time_iterations call")
    ap.add_argument("--parity-cycles", type=int, default=60, help="cap of the parity-mode V-cycle loop (0: skip it)")
    ap.add_argument("--pmax", type=int, default=None,
                    help="cap on the entries per row of P (sets SSS_SETUP_PMAX; DESIGN.md 6.9); 0: no cap, but the "
                         "truncation's own seconds are reported as with a cap")
    ap.add_argument("--no-forced", action="store_true", help="skip the setups forced to the device and to the host")
    ap.add_argument("--no-solve", action="store_true", help="stop after the forced setups")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if A.device_count() < 1:
        print("no HIP device visible", file=sys.stderr)
        return 1
    os.environ["SSS_SETUP_TIMING"] = "1"
    if args.pmax is not None:
        os.environ["SSS_SETUP_PMAX"] = str(args.pmax)
    n = args.n ** 3
    res = {"problem": f"7-pt {args.n}^3", "rows": n, "split": "PMIS", "pmax": A.setup_pmax(), "mode": "hybrid/direct", "tol": args.tol,
           "host_threads": int(os.environ.get("OMP_NUM_THREADS", os.cpu_count())), "weights_per_level": {}, "variants": {}}
    M = A.generate(7, args.n)   # stays alive: level 0 of every hierarchy copies it

    # the weights of every level, forced to the device and to the host
    for name, interp in ({} if args.no_forced else VARIANTS).items():
        per, nnz = {}, None
        for where, env in (("device", {ENV[0]: "1", ENV[1]: "0"}), ("host", {ENV[0]: "0"})):
            with environment(**env):
                t0 = time.perf_counter()
                with capture_fds() as cap:
                    H = A.Hierarchy(M, make_pars(A.COARSE_PMIS, interp))
                wall = time.perf_counter() - t0
            nnz = [H.level(l).A.num_nnzs for l in range(H.num_levels)]
            H.close()
            per[where] = weight_lines(cap.text)
            assert per[where] and all(r["where"] == where for r in per[where]), (name, where, per[where])
            print(f"[exti] {name}, every level on the {where}: setup {wall:.2f} s", file=sys.stderr, flush=True)
        res["weights_per_level"][name] = []
        for l, (d, h) in enumerate(zip(per["device"], per["host"])):
            assert d["rows"] == h["rows"] and d["entries"] == h["entries"], (name, l)
            res["weights_per_level"][name].append({
                "level": l, "rows": d["rows"], "nnz_A": nnz[l] if l < len(nnz) else None, "nnz_P": d["entries"],
                "lanes": d["lanes"], "global_rows": d["global_rows"], "device_s": d["seconds"], "copies_s": d["copies_s"],
                "kernels_s": d["kernels_s"], "host_s": h["seconds"], "trunc_lanes": d.get("trunc_lanes"),
                "device_trunc_s": d.get("trunc_s"), "host_trunc_s": h.get("trunc_s"),
                "nnz_P_before_truncation": h.get("trunc_entries_before")})

    if args.no_solve:
        return finish(res, args)

    # the two hierarchies in throughput mode
    b = np.random.default_rng(1).standard_normal(n)
    nb = float(np.linalg.norm(b))
    x0 = np.zeros(n)
    devs = {}
    for name, interp in VARIANTS.items():
        t0 = time.perf_counter()
        with capture_fds() as cap:
            D = A.DeviceHierarchy(None, setup_from=M, pars=make_pars(A.COARSE_PMIS, interp), smoother="hybrid",
                                  coarse="direct")
        wall = time.perf_counter() - t0
        devs[name] = D
        info = [D.level_info(l) for l in range(D.H.num_levels)]
        res["variants"][name] = {
            "setup_s": D.times[0], "mirror_after_s": D.times[1], "create_wall_s": wall, "levels": D.H.num_levels,
            "rows": [i.rows for i in info], "nnz": [i.nnz for i in info],
            "nnz_P": [D.H.level(l).P.num_nnzs for l in range(D.H.num_levels - 1)],
            "operator_complexity": sum(i.nnz for i in info) / info[0].nnz,
            "phase_lines": [l for l in cap.text.splitlines() if l.startswith("[setup]")]}
        v = res["variants"][name]
        v["p_per_level"] = []
        for l in range(D.H.num_levels - 1):
            L = D.H.level(l)
            rp, _, val = A.csr_arrays(L.P, copy=False)
            cf = np.ctypeslib.as_array(L.cfmark.d, shape=(L.A.num_rows,))
            v["p_per_level"].append({"level": l, "max_abs_p": float(np.abs(val).max()), "longest_row": int(np.diff(rp).max()),
                                     "f_rows_without_pattern": int(((np.diff(rp) == 0) & (cf == 0)).sum()),
                                     "isolated_rows": int((cf == 2).sum())})
        print(f"[exti] {name}: setup {v['setup_s']:.2f} + mirror {v['mirror_after_s']:.2f} s, rows {v['rows']}, "
              f"opc {v['operator_complexity']:.3f}", file=sys.stderr, flush=True)

    ms = {name: [] for name in devs}
    for D in devs.values():   # warm-up: graph capture
        D.upload(0, "b", b)
        D.upload(0, "x", x0)
        D.time_iterations(2)
    for _ in range(max(3, args.reps)):
        for name, D in devs.items():
            D.upload(0, "x", x0)
            ms[name].append(D.time_iterations(args.iters)[0])
    for name in devs:
        res["variants"][name]["ms_per_iteration"] = {"median": statistics.median(ms[name]), "min": min(ms[name]),
                                                     "max": max(ms[name]), "samples": ms[name]}

    for name, D in devs.items():
        v = res["variants"][name]

        def vcycle():
            rel = []
            while len(rel) < args.maxit:
                D.cycle()
                rel.append(D.residual_norm() / nb)
                if rel[-1] < args.tol or not rel[-1] < 1e6:   # converged, or diverging
                    break
            return len(rel), rel

        for solver, fn in (("vcycle", vcycle), ("pcg", lambda: D.pcg(args.tol, args.maxit))):
            runs = []
            for _ in range(2):   # the first run warms up, the second is timed
                D.upload(0, "b", b)
                D.upload(0, "x", x0)
                D.sync()
                t0 = time.perf_counter()
                its, hist = fn()
                D.sync()
                dt = time.perf_counter() - t0
                runs.append({"iterations": int(its), "seconds": dt, "last_relres": float(hist[-1]),
                             "true_relres": D.residual_norm() / nb})
            v[solver] = runs[1]
            v[solver + "_operator_to_answer_s"] = v["setup_s"] + v["mirror_after_s"] + runs[1]["seconds"]
        print(f"[exti] {name}: vcycle {v['vcycle']}, pcg {v['pcg']}", file=sys.stderr, flush=True)
    for D in devs.values():
        D.close()

    # the same hierarchies in parity mode: the V-cycle loop
    for name, D in devs.items():
        if args.parity_cycles > 0:
            with capture_fds():
                E = A.DeviceHierarchy(D.H, smoother="exact", coarse="krylov")
            E.upload(0, "b", b)
            E.upload(0, "x", x0)
            rel = []
            while len(rel) < args.parity_cycles:
                E.cycle()
                rel.append(E.residual_norm() / nb)
                if rel[-1] < args.tol or not rel[-1] < 1e6:
                    break
            E.close()
            res["variants"][name]["parity_vcycle"] = {"iterations": len(rel), "converged": bool(rel[-1] < args.tol),
                                                      "relres": rel}
            print(f"[exti] {name}: parity mode {len(rel)} cycles, relres {rel[-1]:.3e}", file=sys.stderr, flush=True)
        D.H.close()

    return finish(res, args)


def finish(res, args) -> int:
    text = json.dumps(res, indent=1)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
