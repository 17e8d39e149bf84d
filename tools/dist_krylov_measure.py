#!/usr/bin/env python
"""Measurements for DESIGN.md §7.1 (Krylov solvers on the row-partitioned engine), one process, one GPU:

- the fused level-0 kernels (pcg_update + dot2_partials and their final sums) against the chain of
  launch_axpy_ratio / copy / launch_dot they replace, at --lab-n rows (sss_lab_time_pcg_fused:
  device events, the two alternating rep by rep on the same vectors);
- whole solves of the 7-point n^3 problem in throughput mode (hybrid smoother, direct coarse solve,
  free-order sums; b = 1, x0 = 0) to --tol: DistHierarchy.pcg at world 1 over RCCL, the distributed
  V-cycle loop (cycle + residual_norm) and the single-GPU sss_hip_pcg.  Each is run once to warm up
  (graph capture, workspace allocation) and then timed --solve-reps times with a host clock around
  calls that end in a stream synchronise; the median is reported beside every single time (the
  spread of a 50 ms window);
- the same for DistHierarchy.fgmres at world 1 over RCCL and the single-GPU sss_hip_fgmres (--restart);
- the reductions' share of a PCG iteration: the same solve with the timing communicator, which
  skips every collective (at world 1 a skipped reduction is the identity, so the iterates are the
  same) -- the difference per iteration is what the three ncclAllReduce calls cost.

N > 1 over xGMI is not measured here.  Writes one JSON document to --out and prints it.  Needs a GPU.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import socket
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import amg_amd as A  # noqa: E402


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, time.perf_counter() - t0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--lab-n", type=int, default=1 << 24)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--maxit", type=int, default=100)
    ap.add_argument("--restart", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--solve-reps", type=int, default=7)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if A.device_count() < 1:
        print("no HIP device visible", file=sys.stderr)
        return 1
    lib = A.lib()
    lib.sss_lab_time_pcg_fused.restype = C.c_int
    lib.sss_lab_time_pcg_fused.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    res = {"problem": f"7-pt {args.n}^3", "mode": "hybrid/direct, sum_order 1", "tol": args.tol}

    f, c = C.c_double(), C.c_double()
    rc = lib.sss_lab_time_pcg_fused(args.lab_n, args.reps, C.byref(f), C.byref(c))
    if rc != 0:
        print(f"sss_lab_time_pcg_fused failed ({rc})", file=sys.stderr)
        return 1
    nb = 8 * args.lab_n
    res["vector_work"] = {"rows": args.lab_n, "fused_ms": f.value, "chain_ms": c.value, "fused_over_chain": f.value / c.value,
                          # fused 56 + 24 B per row; chain 2 x 24 (axpy) + 16 (copy) + 3 x 16 (dot)
                          "fused_model_bytes": 10 * nb, "chain_model_bytes": 14 * nb,
                          "fused_GBps": 10 * nb / f.value / 1e6, "chain_GBps": 14 * nb / c.value / 1e6}
    print(f"[vector work] {res['vector_work']}", file=sys.stderr, flush=True)

    M = A.generate(7, args.n)   # stays alive: level 0 of the hierarchy is this operator
    H, t_setup = timed(lambda: A.Hierarchy(M))
    N = M.num_rows
    res["setup_s"] = t_setup
    mode = dict(smoother="hybrid", coarse="direct", sum_order=1)
    b, x0 = np.ones(N), np.zeros(N)

    def start(E, dist):
        if dist:
            E.upload("b", b)
            E.upload("x", x0)
        else:
            E.upload(0, "b", b)
            E.upload(0, "x", x0)
        E.sync()

    def pcg_timed(E, dist, solver="pcg"):
        solve = (lambda: E.pcg(args.tol, args.maxit)) if solver == "pcg" else \
            (lambda: E.fgmres(args.tol, args.restart, args.maxit))
        start(E, dist)
        solve()   # warm-up
        ts = []
        for _ in range(args.solve_reps):
            start(E, dist)
            (its, hist), t = timed(solve)
            ts.append(t)
        t = float(np.median(ts))
        return {"iterations": its, "seconds": t, "all_seconds": ts, "ms_per_iteration": 1e3 * t / max(its, 1),
                "relres": float(hist[-1])}

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=0, world_size=1)

    comm = A.Comm(1, 0, "rccl", device=0)
    D = A.DistHierarchy(H, comm, device=0, **mode)
    res["dist_pcg_rccl"] = pcg_timed(D, True)
    res["dist_cycle_graph"] = D.level_flags(0)["cycle_graph"]
    res["dist_fgmres_rccl"] = pcg_timed(D, True, "fgmres")
    print(f"[dist fgmres] {res['dist_fgmres_rccl']}", file=sys.stderr, flush=True)
    print(f"[dist pcg] {res['dist_pcg_rccl']}", file=sys.stderr, flush=True)

    def vloop():
        rel = []
        while len(rel) < args.maxit:
            D.cycle()
            rel.append(D.residual_norm() / np.sqrt(N))
            if rel[-1] < args.tol:
                break
        return rel
    start(D, True)
    vloop()
    ts = []
    for _ in range(args.solve_reps):
        start(D, True)
        rel, t = timed(vloop)
        ts.append(t)
    t = float(np.median(ts))
    res["dist_vcycle_loop"] = {"iterations": len(rel), "seconds": t, "all_seconds": ts, "ms_per_iteration": 1e3 * t / len(rel),
                               "relres": float(rel[-1])}
    print(f"[dist V-cycle loop] {res['dist_vcycle_loop']}", file=sys.stderr, flush=True)
    D.close()
    comm.close()

    comm = A.Comm(1, 0, "timing", device=0)
    D = A.DistHierarchy(H, comm, device=0, **mode)
    res["dist_pcg_no_collectives"] = pcg_timed(D, True)
    D.close()
    comm.close()
    a, z = res["dist_pcg_rccl"], res["dist_pcg_no_collectives"]
    if a["iterations"] == z["iterations"]:
        d = a["ms_per_iteration"] - z["ms_per_iteration"]
        res["reductions"] = {"ms_per_iteration": d, "share_of_iteration": d / a["ms_per_iteration"]}
    print(f"[dist pcg, collectives skipped] {z}  reductions: {res.get('reductions')}", file=sys.stderr, flush=True)

    S = A.DeviceHierarchy(H, device=0, **mode)
    res["single_gpu_pcg"] = pcg_timed(S, False)
    res["single_gpu_fgmres"] = pcg_timed(S, False, "fgmres")
    S.close()
    print(f"[single-GPU pcg] {res['single_gpu_pcg']}\n[single-GPU fgmres] {res['single_gpu_fgmres']}", file=sys.stderr, flush=True)
    dist.destroy_process_group()

    text = json.dumps(res, indent=1)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
