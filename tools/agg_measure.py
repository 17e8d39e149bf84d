#!/usr/bin/env python
"""Measurements for DESIGN.md 6.8 (aggressive PMIS coarsening with multipass interpolation, cs_type 4), one
process, one GPU, 7-point or 27-point n^3, cs_type 3 + interp_type 2 against cs_type 4:

  - two host-only setups (SSS_amg_setup) with cs_type 4, the aggressive level's steps forced to the device
    (SSS_SETUP_GPU_AGG, SSS_SETUP_GPU_PMIS and SSS_SETUP_GPU_INTERP on with thresholds 0) and to the host:
    per step (S2, the stage-two split, the multipass P) the seconds of either side, the device's split into
    copies and kernels where the step reports them;
  - per variant one setup + mirror (sss_hip_setup_create, throughput mode: hybrid smoother, direct coarse
    solve) at the library's thresholds: setup and mirror seconds, rows and nonzeros per level, operator
    complexity, HBM in use, ms per iteration (the hierarchies alternated sample by sample), V-cycle and PCG
    iterations to --tol with their wall times (b = standard_normal, seed 1, x0 = 0), and setup + mirror +
    solve: operator to answer.

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
from pmis_measure import capture_fds, make_pars  # noqa: E402

VARIANTS = {"pmis_interp2": A.COARSE_PMIS, "pmis_agg": A.COARSE_PMIS_AGG}
SWITCHES = ("SSS_SETUP_GPU_AGG", "SSS_SETUP_GPU_PMIS", "SSS_SETUP_GPU_INTERP")
STEPS = {
    "s2": (re.compile(r"aggressive S2: device, (\d+) rows, (\d+) entries, (\d+) lanes per row, (\d+) rows on global tables, "
                      r"copies ([0-9.]+) s, kernels ([0-9.]+) s"),
           re.compile(r"aggressive S2: host ([0-9.]+) s, (\d+) rows, (\d+) entries")),
    "multipass": (re.compile(r"multipass P: device, (\d+) passes, (\d+) rows unreached, (\d+) rows, (\d+) entries, up to (\d+) "
                             r"lanes per row, (\d+) rows on global tables, copies ([0-9.]+) s, kernels ([0-9.]+) s"),
                  re.compile(r"multipass P: host ([0-9.]+) s, (\d+) passes, (\d+) rows unreached, (\d+) rows, (\d+) entries")),
}
SPLIT2 = re.compile(r"aggressive stage-two split: (device|host) ([0-9.]+) s, (\d+) rounds, (\d+) rows, (\d+) entries")


class switches:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        names = [s + t for s in SWITCHES for t in ("", "_MIN")]
        self.saved = {k: os.environ.get(k) for k in names}
        for s in SWITCHES:
            os.environ[s] = "1" if self.on else "0"
            if self.on:
                os.environ[s + "_MIN"] = "0"
            else:
                os.environ.pop(s + "_MIN", None)

    def __exit__(self, *a):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def step_lines(text: str) -> dict:
    out = {}
    m = STEPS["s2"][0].search(text)
    if m:
        out["s2"] = {"where": "device", "rows": int(m.group(1)), "entries": int(m.group(2)), "lanes": int(m.group(3)),
                     "global_rows": int(m.group(4)), "copies_s": float(m.group(5)), "kernels_s": float(m.group(6)),
                     "seconds": float(m.group(5)) + float(m.group(6))}
    m = STEPS["s2"][1].search(text)
    if m:
        out["s2"] = {"where": "host", "seconds": float(m.group(1)), "rows": int(m.group(2)), "entries": int(m.group(3))}
    m = STEPS["multipass"][0].search(text)
    if m:
        out["multipass"] = {"where": "device", "passes": int(m.group(1)), "unreached": int(m.group(2)), "rows": int(m.group(3)),
                            "entries": int(m.group(4)), "lanes": int(m.group(5)), "global_rows": int(m.group(6)),
                            "copies_s": float(m.group(7)), "kernels_s": float(m.group(8)),
                            "seconds": float(m.group(7)) + float(m.group(8))}
    m = STEPS["multipass"][1].search(text)
    if m:
        out["multipass"] = {"where": "host", "seconds": float(m.group(1)), "passes": int(m.group(2)), "unreached": int(m.group(3)),
                            "rows": int(m.group(4)), "entries": int(m.group(5))}
    m = SPLIT2.search(text)
    if m:
        out["stage_two_split"] = {"where": m.group(1), "seconds": float(m.group(2)), "rounds": int(m.group(3)),
                                  "rows": int(m.group(4)), "entries": int(m.group(5))}
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", type=int, default=7, choices=(7, 27))
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--maxit", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5, help="alternated timing samples per hierarchy (at least 3)")
    ap.add_argument("--iters", type=int, default=10, help="iterations per time_iterations call")
    ap.add_argument("--skip-steps", action="store_true", help="skip the forced host / device setups")
    ap.add_argument("--pmax", type=int, default=None,
                    help="cap on the entries per row of P (sets SSS_SETUP_PMAX; DESIGN.md 6.9)")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if A.device_count() < 1:
        print("no HIP device visible", file=sys.stderr)
        return 1
    os.environ["SSS_SETUP_TIMING"] = "1"
    if args.pmax is not None:
        os.environ["SSS_SETUP_PMAX"] = str(args.pmax)
    n = args.n ** 3
    res = {"problem": f"{args.kind}-pt {args.n}^3", "rows": n, "pmax": A.setup_pmax(), "mode": "hybrid/direct", "tol": args.tol,
           "host_threads": int(os.environ.get("OMP_NUM_THREADS", os.cpu_count())), "steps": {}, "variants": {}}
    M = A.generate(args.kind, args.n)   # stays alive: level 0 of every hierarchy copies it

    if not args.skip_steps:
        for where in ("device", "host"):
            with switches(where == "device"):
                t0 = time.perf_counter()
                with capture_fds() as cap:
                    H = A.Hierarchy(M, make_pars(A.COARSE_PMIS_AGG, 2))
                wall = time.perf_counter() - t0
            H.close()
            res["steps"][where] = step_lines(cap.text)
            res["steps"][where]["setup_wall_s"] = wall
            print(f"[agg] cs_type 4, the aggressive level on the {where}: setup {wall:.2f} s, {res['steps'][where]}",
                  file=sys.stderr, flush=True)

    b = np.random.default_rng(1).standard_normal(n)
    nb = float(np.linalg.norm(b))
    x0 = np.zeros(n)
    devs = {}
    for name, cs in VARIANTS.items():
        before = A.hbm_used_bytes()
        t0 = time.perf_counter()
        with capture_fds() as cap:
            D = A.DeviceHierarchy(None, setup_from=M, pars=make_pars(cs, 2), smoother="hybrid", coarse="direct")
        wall = time.perf_counter() - t0
        devs[name] = D
        info = [D.level_info(l) for l in range(D.H.num_levels)]
        res["variants"][name] = {
            "setup_s": D.times[0], "mirror_after_s": D.times[1], "create_wall_s": wall, "levels": D.H.num_levels,
            "rows": [i.rows for i in info], "nnz": [i.nnz for i in info],
            "nnz_P": [D.H.level(l).P.num_nnzs for l in range(D.H.num_levels - 1)],
            "operator_complexity": sum(i.nnz for i in info) / info[0].nnz,
            "hbm_bytes": A.hbm_used_bytes() - before,
            "phase_lines": [l for l in cap.text.splitlines() if l.startswith("[setup]")]}
        v = res["variants"][name]
        print(f"[agg] {name}: setup {v['setup_s']:.2f} + mirror {v['mirror_after_s']:.2f} s, rows {v['rows']}, "
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
        print(f"[agg] {name}: vcycle {v['vcycle']}, pcg {v['pcg']}", file=sys.stderr, flush=True)
    for D in devs.values():
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
