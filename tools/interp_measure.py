#!/usr/bin/env python
"""Measurements for DESIGN.md 6.5 (the standard interpolation's pattern and weights on the device), one
process, one GPU, 7-point n^3, PMIS + interp_type 2:

  - two host-only setups (SSS_amg_setup) of the same operator, every level's pattern and weights
    forced to the device (SSS_SETUP_GPU_INTERP=1, SSS_SETUP_GPU_INTERP_MIN=0) and to the host
    (SSS_SETUP_GPU_INTERP=0): per level rows, nnz(A), nnz of the pattern and of P, the device seconds
    with copies and kernels split, the host seconds (OpenMP, the threads of this process);
  - setup + mirror (sss_hip_setup_create, throughput mode) with the device path off and on at the
    library's threshold, with the SSS_SETUP_TIMING phase lines kept verbatim, and a warmed-up PCG
    solve to --tol on each (b = standard_normal, seed 1, x0 = 0): operator to answer.

Writes one JSON document to --out and prints it.  Needs a GPU; there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import amg_amd as A  # noqa: E402
from pmis_measure import capture_fds, make_pars  # noqa: E402

ENV = ("SSS_SETUP_GPU_INTERP", "SSS_SETUP_GPU_INTERP_MIN")
DEV = re.compile(r"standard P: device (pattern|weights), (\d+) rows, (\d+) entries, (\d+) lanes per row, "
                 r"(\d+) rows on global tables, copies ([0-9.]+) s, kernels ([0-9.]+) s")
HOST = re.compile(r"standard P: host (pattern|weights) ([0-9.]+) s, (\d+) rows, (\d+) entries")


class environment:
    def __init__(self, **env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in ENV}
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def step_lines(text: str) -> dict:
    """step -> one record per level, from the timing lines of one setup."""
    out = {"pattern": [], "weights": []}
    for line in text.splitlines():
        m = DEV.search(line)
        if m:
            out[m.group(1)].append({"where": "device", "rows": int(m.group(2)), "entries": int(m.group(3)),
                                    "lanes": int(m.group(4)), "global_rows": int(m.group(5)), "copies_s": float(m.group(6)),
                                    "kernels_s": float(m.group(7)), "seconds": float(m.group(6)) + float(m.group(7))})
        m = HOST.search(line)
        if m:
            out[m.group(1)].append({"where": "host", "rows": int(m.group(3)), "entries": int(m.group(4)),
                                    "seconds": float(m.group(2))})
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--maxit", type=int, default=100)
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--no-mirror", action="store_true", help="skip the two setup + mirror runs")
    args = ap.parse_args()
    if A.device_count() < 1:
        print("no HIP device visible", file=sys.stderr)
        return 1
    os.environ["SSS_SETUP_TIMING"] = "1"
    pars = lambda: make_pars(A.COARSE_PMIS, 2)  # noqa: E731
    res = {"problem": f"7-pt {args.n}^3", "rows": args.n ** 3, "split": "PMIS", "interp_type": 2,
           "host_threads": int(os.environ.get("OMP_NUM_THREADS", os.cpu_count()))}
    M = A.generate(7, args.n)   # stays alive: level 0 of every hierarchy copies it

    per, setup_s = {}, {}
    for where, env in (("device", {ENV[0]: "1", ENV[1]: "0"}), ("host", {ENV[0]: "0"})):
        with environment(**env):
            t0 = time.perf_counter()
            with capture_fds() as cap:
                H = A.Hierarchy(M, pars())
            setup_s[where] = time.perf_counter() - t0
        nnz = [H.level(l).A.num_nnzs for l in range(H.num_levels)]
        H.close()
        per[where] = step_lines(cap.text)
        for step, recs in per[where].items():
            assert recs and all(r["where"] == where for r in recs), (where, step, recs)
        print(f"[interp] every level on the {where}: setup {setup_s[where]:.2f} s", file=sys.stderr, flush=True)
    res["setup_all_levels_s"] = setup_s
    res["per_level"] = []
    for l, (dp, dw, hp, hw) in enumerate(zip(per["device"]["pattern"], per["device"]["weights"], per["host"]["pattern"],
                                            per["host"]["weights"])):
        assert dp["rows"] == hp["rows"] and dp["entries"] == hp["entries"] and dw["entries"] == hw["entries"], l
        res["per_level"].append({
            "level": l, "rows": dp["rows"], "nnz_A": nnz[l] if l < len(nnz) else None, "nnz_pattern": dp["entries"],
            "nnz_P": dw["entries"], "lanes": dp["lanes"], "global_rows": dp["global_rows"],
            "pattern": {"device_s": dp["seconds"], "copies_s": dp["copies_s"], "kernels_s": dp["kernels_s"],
                        "host_s": hp["seconds"]},
            "weights": {"device_s": dw["seconds"], "copies_s": dw["copies_s"], "kernels_s": dw["kernels_s"],
                        "host_s": hw["seconds"]}})

    if not args.no_mirror:
        res["setup_and_mirror"] = {}
        for name, env in (("device_path_off", {ENV[0]: "0"}), ("device_path_on", {ENV[0]: "1"})):
            with environment(**env):
                t0 = time.perf_counter()
                with capture_fds() as cap:
                    D = A.DeviceHierarchy(None, setup_from=M, pars=pars(), smoother="hybrid", coarse="direct")
                wall = time.perf_counter() - t0
            steps = step_lines(cap.text)
            res["setup_and_mirror"][name] = {
                "setup_s": D.times[0], "mirror_after_s": D.times[1], "create_wall_s": wall, "levels": D.H.num_levels,
                "where": {s: [r["where"] for r in recs] for s, recs in steps.items()},
                "phase_lines": [l for l in cap.text.splitlines() if l.startswith("[setup]")]}
            b = np.random.default_rng(1).standard_normal(args.n ** 3)
            for _ in range(2):   # the first run warms up, the second is timed
                D.upload(0, "b", b)
                D.upload(0, "x", np.zeros(args.n ** 3))
                D.sync()
                t0 = time.perf_counter()
                its, hist = D.pcg(args.tol, args.maxit)
                D.sync()
                solve = time.perf_counter() - t0
            v = res["setup_and_mirror"][name]
            v["pcg"] = {"iterations": int(its), "seconds": solve, "last_relres": float(hist[-1])}
            v["pcg_operator_to_answer_s"] = v["setup_s"] + v["mirror_after_s"] + solve
            print(f"[interp] {name}: setup {D.times[0]:.2f} + mirror {D.times[1]:.2f} s, pcg {its} its {solve:.3f} s",
                  file=sys.stderr, flush=True)
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
