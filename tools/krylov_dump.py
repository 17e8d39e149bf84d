"""Results of the Krylov solvers on a fixed list of small cases, one .npz per case (iters, relres,
hist, x -- or w, hcol, norm for the orthogonalisation step), saved for a bitwise A/B of two builds of
the library (SSS_AMG_LIB selects the one loaded).

    python tools/krylov_dump.py --out DIR            # needs a GPU
    python tools/krylov_dump.py --compare DIR_A DIR_B   # every array identical as uint64, every count equal

Right-hand side default_rng(1).standard_normal(N), x0 = 0, tol 1e-6.  The partitioned solvers run at
world 1 over RCCL.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import socket
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

TOL = 1e-6
MODES = {"hybrid": dict(smoother="hybrid", coarse="direct"), "exact": dict(smoother="exact", coarse="krylov")}
ORTH = [(1, 1), (63, 7), (1331, 9), (4097, 21)]   # seeds as tests/test_gpu_fgmres.py: 1000 n + k


def quiet_hierarchy(A, mat):
    saved = os.dup(1)
    os.dup2(2, 1)
    try:
        return A.Hierarchy(mat)
    finally:
        C.CDLL(None).fflush(None)
        os.dup2(saved, 1)
        os.close(saved)


def dump(out: Path):
    import amg_amd as A
    from amg_amd._native import dptr

    lib = A.lib()
    out.mkdir(parents=True, exist_ok=True)
    hiers = {}

    def hier(kind, n):
        if (kind, n) not in hiers:
            M = A.convdiff_csr(n, 2.0) if kind == "convdiff" else A.generate(kind, n)
            hiers[(kind, n)] = (M, quiet_hierarchy(A, M.mat if kind == "convdiff" else M))   # M stays alive
        return hiers[(kind, n)][1]

    def save(name, its, rel, hist, x):
        np.savez(out / f"{name}.npz", iters=np.int64(its), relres=np.float64(rel), hist=hist, x=x)
        print(f"{name}: {its} iterations, relres {rel:.17g}", flush=True)

    def single(name, kind, n, mode, solver, restart=20, maxit=100):
        H = hier(kind, n)
        N = H.level(0).A.num_rows
        D = A.DeviceHierarchy(H, **MODES[mode])
        D.upload(0, "b", np.random.default_rng(1).standard_normal(N))
        D.upload(0, "x", np.zeros(N))
        hist = np.zeros(maxit)
        its, rel = C.c_int(), C.c_double()
        if solver == "fgmres":
            rc = lib.sss_hip_fgmres(D.h, TOL, restart, maxit, C.byref(its), C.byref(rel), dptr(hist), maxit)
        else:
            rc = lib.sss_hip_pcg(D.h, TOL, maxit, C.byref(its), C.byref(rel), dptr(hist), maxit)
        assert rc == 0, (name, rc)
        save(name, its.value, rel.value, hist[: its.value], D.download(0, "x"))
        D.close()

    for n in (11, 16):
        for restart in (3, 20):
            for mode in MODES:
                single(f"fgmres_convdiff{n}_m{restart}_{mode}", "convdiff", n, mode, "fgmres", restart)
    single("fgmres_p7_24_m20_hybrid", 7, 24, "hybrid", "fgmres", 20)
    single("fgmres_convdiff16_m3_maxit4_hybrid", "convdiff", 16, "hybrid", "fgmres", 3, 4)
    single("pcg_p7_24_hybrid", 7, 24, "hybrid", "pcg")
    single("pcg_p27_14_hybrid", 27, 14, "hybrid", "pcg")

    for n, k in ORTH:
        rng = np.random.default_rng(1000 * n + k)
        Q, _ = np.linalg.qr(rng.standard_normal((n, k)))
        V = np.ascontiguousarray(Q.T)
        w, h, nrm = rng.standard_normal(n), np.zeros(k), np.zeros(1)
        assert lib.sss_hip_host_orth(n, k, dptr(V), dptr(w), dptr(h), dptr(nrm)) == 0
        np.savez(out / f"orth_n{n}_k{k}.npz", w=w, hcol=h, norm=nrm)
        print(f"orth_n{n}_k{k}: norm {nrm[0]:.17g}", flush=True)

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=0, world_size=1)
    comm = A.Comm(1, 0, "rccl", device=0)
    for kind, n, smoother in ((7, 24, "hybrid"), ("convdiff", 16, "jacobi")):
        H = hier(kind, n)
        N = H.level(0).A.num_rows
        D = A.DistHierarchy(H, comm, agg_rows=100, smoother=smoother, coarse="direct", device=0)
        for solver in ("fgmres", "pcg"):
            D.upload("b", np.random.default_rng(1).standard_normal(N))
            D.upload("x", np.zeros(N))
            hist = np.zeros(100)
            its, rel = C.c_int(), C.c_double()
            if solver == "fgmres":
                rc = lib.sss_hip_dist_fgmres(D.d, TOL, 20, 100, C.byref(its), C.byref(rel), dptr(hist), 100)
            else:
                rc = lib.sss_hip_dist_pcg(D.d, TOL, 100, C.byref(its), C.byref(rel), dptr(hist), 100)
            name = f"dist_{solver}_{'convdiff' if kind == 'convdiff' else 'p%d' % kind}{n}_{smoother}"
            if rc != 0:   # (PCG on the nonsymmetric operator may stop on a non-finite norm: the code is the result)
                np.savez(out / f"{name}.npz", rc=np.int64(rc), iters=np.int64(its.value), x=D.download("x"))
                print(f"{name}: rc {rc} after {its.value} iterations", flush=True)
                continue
            save(name, its.value, rel.value, hist[: its.value], D.download("x"))
        D.close()
    comm.close()
    dist.destroy_process_group()


def compare(a: Path, b: Path) -> int:
    names = sorted(p.name for p in a.glob("*.npz"))
    bad = 0
    if names != sorted(p.name for p in b.glob("*.npz")) or not names:
        print("the two directories hold different cases")
        return 1
    for name in names:
        za, zb = np.load(a / name), np.load(b / name)
        diff = [k for k in sorted(set(za.files) | set(zb.files))
                if k not in za.files or k not in zb.files or za[k].shape != zb[k].shape
                or not np.array_equal(np.atleast_1d(za[k]).view(np.uint64), np.atleast_1d(zb[k]).view(np.uint64))]
        print(f"{name}: {'identical' if not diff else 'DIFFERS in ' + ', '.join(diff)}"
              f" ({', '.join(f'{k}{list(za[k].shape)}' for k in za.files)})")
        bad += bool(diff)
    print(f"{len(names)} cases, {bad} differ")
    return 1 if bad else 0


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--out", type=Path)
    p.add_argument("--compare", type=Path, nargs=2)
    a = p.parse_args()
    if a.compare:
        return compare(*a.compare)
    if not a.out:
        p.error("--out or --compare")
    dump(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
