#!/usr/bin/env python
"""Measurements for DESIGN.md "PMIS coarsening" (cs_type 3), one process, one GPU, 7-point n^3:

three setups of the same operator -- RS + interp_type 1 (the default), RS + interp_type 2, PMIS +
interp_type 2 -- each through sss_hip_setup_create (throughput mode: hybrid smoother, direct coarse
solve), with per variant
  - the SSS_SETUP_TIMING phase lines (the library's stderr, kept verbatim),
  - setup seconds and the mirror seconds after it, levels, rows per level, operator complexity,
  - ms per iteration (time_iterations, the variants alternated rep by rep: median, min, max),
  - V-cycle iterations and PCG iterations to --tol with their wall times (b = standard_normal, seed 1,
    x0 = 0), and the sum setup + mirror + solve: operator to answer;
and the PMIS split's time per level on the device (upload and download included) and on the host,
from two more setups with SSS_SETUP_GPU_PMIS_MIN=0 and SSS_SETUP_GPU_PMIS=0.

Writes one JSON document to --out and prints it.  Needs a GPU; there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import amg_amd as A  # noqa: E402

VARIANTS = {"rs_interp1": (A.COARSE_RS, 1), "rs_interp2": (A.COARSE_RS, 2), "pmis_interp2": (A.COARSE_PMIS, 2)}


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
        import ctypes
        ctypes.CDLL(None).fflush(None)
        os.dup2(self.saved[0], 1)
        os.dup2(self.saved[1], 2)
        for fd in self.saved:
            os.close(fd)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def make_pars(cs_type: int, interp_type: int):
    p = A.default_pars()
    p.cs_type, p.interp_type = cs_type, interp_type
    return p


def split_lines(text: str) -> list:
    """The PMIS split line of each level: where it ran, drop and split seconds, rounds, entries of S."""
    pat = re.compile(r"PMIS split: drop ([0-9.]+) s, (device|host) split ([0-9.]+) s, (\d+) rounds, (\d+) strong entries")
    return [{"where": m.group(2), "drop_s": float(m.group(1)), "split_s": float(m.group(3)), "rounds": int(m.group(4)),
             "strong_entries": int(m.group(5))} for m in pat.finditer(text)]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--maxit", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5, help="alternated timing repetitions per variant (at least 3)")
    ap.add_argument("--iters", type=int, default=10, help="iterations per time_iterations call")
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if A.device_count() < 1:
        print("no HIP device visible", file=sys.stderr)
        return 1
    os.environ["SSS_SETUP_TIMING"] = "1"
    names = [v for v in args.variants.split(",") if v]
    n = args.n ** 3
    res = {"problem": f"7-pt {args.n}^3", "rows": n, "mode": "hybrid/direct", "tol": args.tol,
           "pmis_min_default": os.environ.get("SSS_SETUP_GPU_PMIS_MIN", "library default"), "variants": {}}
    M = A.generate(7, args.n)   # stays alive: level 0 of every hierarchy copies it
    b = np.random.default_rng(1).standard_normal(n)
    nb = float(np.linalg.norm(b))
    x0 = np.zeros(n)

    devs = {}
    for name in names:
        t0 = time.perf_counter()
        with capture_fds() as cap:
            D = A.DeviceHierarchy(None, setup_from=M, pars=make_pars(*VARIANTS[name]), smoother="hybrid", coarse="direct")
        wall = time.perf_counter() - t0
        devs[name] = D
        nl = D.H.num_levels
        info = [D.level_info(l) for l in range(nl)]
        v = {"setup_s": D.times[0], "mirror_after_s": D.times[1], "create_wall_s": wall, "levels": nl,
             "rows": [i.rows for i in info], "nnz": [i.nnz for i in info],
             "operator_complexity": sum(i.nnz for i in info) / info[0].nnz,
             "phase_lines": [l for l in cap.text.splitlines() if l.startswith("[setup]")]}
        if name.startswith("pmis"):
            v["split_per_level"] = split_lines(cap.text)
        res["variants"][name] = v
        print(f"[setup] {name}: {v['setup_s']:.2f} + {v['mirror_after_s']:.2f} s, rows {v['rows']}, "
              f"opc {v['operator_complexity']:.3f}", file=sys.stderr, flush=True)

    # ms per iteration, the variants alternated
    ms = {name: [] for name in names}
    for name in names:   # warm-up: graph capture
        devs[name].upload(0, "b", b)
        devs[name].upload(0, "x", x0)
        devs[name].time_iterations(2)
    for _ in range(max(3, args.reps)):
        for name in names:
            devs[name].upload(0, "x", x0)
            ms[name].append(devs[name].time_iterations(args.iters)[0])
    for name in names:
        res["variants"][name]["ms_per_iteration"] = {"median": statistics.median(ms[name]), "min": min(ms[name]),
                                                     "max": max(ms[name]), "samples": ms[name]}

    # iterations to tol: the V-cycle loop and PCG (first run warms up, second is timed)
    for name in names:
        D, v = devs[name], res["variants"][name]

        def vcycle():
            rel = []
            while len(rel) < args.maxit:
                D.cycle()
                rel.append(D.residual_norm() / nb)
                if rel[-1] < args.tol:
                    break
            return len(rel), rel

        for solver, fn in (("vcycle", vcycle), ("pcg", lambda: D.pcg(args.tol, args.maxit))):
            runs = []
            for _ in range(2):
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
        print(f"[solve] {name}: vcycle {v['vcycle']}, pcg {v['pcg']}", file=sys.stderr, flush=True)
    for D in devs.values():
        D.close()
        D.H.close()
    devs.clear()

    # the PMIS split per level: every level on the device, then every level on the host
    if "pmis_interp2" in names:
        per = {}
        for where, env in (("device", {"SSS_SETUP_GPU_PMIS": "1", "SSS_SETUP_GPU_PMIS_MIN": "0"}),
                           ("host", {"SSS_SETUP_GPU_PMIS": "0"})):
            saved = {k: os.environ.get(k) for k in ("SSS_SETUP_GPU_PMIS", "SSS_SETUP_GPU_PMIS_MIN")}
            os.environ.update(env)
            with capture_fds() as cap:
                H = A.Hierarchy(M, make_pars(*VARIANTS["pmis_interp2"]))
            H.close()
            for k, val in saved.items():
                if val is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = val
            per[where] = split_lines(cap.text)
            assert all(s["where"] == where for s in per[where]), per[where]
        rows, nnz = res["variants"]["pmis_interp2"]["rows"], res["variants"]["pmis_interp2"]["nnz"]
        res["pmis_split_device_vs_host"] = [
            {"level": l, "rows": rows[l] if l < len(rows) else None, "nnz_A": nnz[l] if l < len(nnz) else None,
             "strong_entries": d["strong_entries"], "rounds": d["rounds"], "device_s": d["split_s"], "host_s": h["split_s"]}
            for l, (d, h) in enumerate(zip(per["device"], per["host"]))]

    text = json.dumps(res, indent=1)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
