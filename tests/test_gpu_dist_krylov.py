"""GPU: AMG-preconditioned CG and flexible GMRES on the row-partitioned engine (sss_hip_dist_pcg,
sss_hip_dist_fgmres) against the single-GPU solvers (sss_hip_pcg, sss_hip_fgmres) in the same mode.

Ranks are spawned as in test_dist_gpu.py (torch.multiprocessing spawn, gloo, the host transport on
device 0; RCCL only at world 1, which is all one GPU allows).  Every rank builds the same hierarchy;
rank 0 also runs the single-GPU engine and compares.  The right-hand side is
default_rng(seed).standard_normal(N), the same on every rank, sliced to the rank's rows; x0 = 0.

Comparison rule (the tolerances of test_gpu_pcg.py and test_gpu_fgmres.py): after
fgmres_restatement.assert_margin has passed on the single-GPU history, the iteration counts are
equal, the histories agree to rtol 1e-6, ||x - x1|| <= 1e-6 ||x1||, the true residual (oracle SpMV
on the host) is below 10 tol for PCG (test_pcg_true_residual_and_speedup) and below tol for FGMRES
(test_fgmres_matches_restatement), and b downloads bitwise unchanged.  The distributed iterates are
not bitwise the single GPU's: the dot products are summed in another order.  Every rank must also
report the same count and the same history (all decisions are taken from reduced values).
"""
from __future__ import annotations

import ctypes as C
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

pytestmark = pytest.mark.gpu

JOIN_TIMEOUT = 300   # the guard against a rank left waiting in a collective the others skipped


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


class _Ctx:
    """One rank's view of a case: the hierarchy, the distributed engine and (rank 0) the single-GPU one."""

    def __init__(self, rank, world, cfg):
        import torch.distributed as dist

        import amg_amd as A
        from conftest import build_hierarchy, quiet_ctx
        from fgmres_restatement import TOL, convdiff_hierarchy

        self.A, self.dist, self.rank, self.world, self.cfg = A, dist, rank, world, cfg
        kind, n = cfg["kind"], cfg["n"]
        if kind == "convdiff":
            self.M, self.H = convdiff_hierarchy(n, 2.0, quiet_ctx)
            self.tol = TOL
        else:
            self.H = build_hierarchy(A.generate(kind, n), quiet_ctx)
            self.tol = self.H.pars.tol
        if cfg.get("solver", "pcg") == "fgmres":
            self.tol = TOL
        self.N = self.H.level(0).A.num_rows
        self.comm = A.Comm(world, rank, cfg.get("transport", "host"), device=0)
        self.mode = dict(smoother=cfg["smoother"], coarse="direct", device=0, inner_from=cfg.get("inner_from", 2))
        if cfg.get("parts"):   # this rank's partition file and the tail file only
            self.D = A.DistHierarchy(None, self.comm, parts=cfg["parts"], **self.mode)
        else:
            self.D = A.DistHierarchy(self.H, self.comm, agg_rows=cfg["agg"], **self.mode)
        assert self.D.nagg >= 2, self.D.nagg
        self.lo, self.hi = self.D.lo, self.D.hi
        self.R = A.DeviceHierarchy(self.H, **self.mode) if rank == 0 else None

    def rhs(self, seed=1):
        return np.random.default_rng(seed).standard_normal(self.N)

    def gather(self, own):
        parts = [None] * self.world
        self.dist.all_gather_object(parts, (self.lo, own))
        x = np.zeros(self.N)
        for lo, xo in parts:
            x[lo:lo + len(xo)] = xo
        return x

    def same_on_every_rank(self, its, hist):
        """The count and the history are computed from reduced values: identical on every rank."""
        got = [None] * self.world
        self.dist.all_gather_object(got, (its, hist.tobytes()))
        assert all(g == got[0] for g in got), [g[0] for g in got]

    def solve_dist(self, b, x0, solver="pcg", **kw):
        D = self.D
        D.upload("b", b[self.lo:self.hi])
        D.upload("x", x0[self.lo:self.hi])
        its, hist = (D.pcg if solver == "pcg" else D.fgmres)(self.tol, **kw)
        b_after = D.download("b")
        assert np.array_equal(_u64(b_after), _u64(b[self.lo:self.hi])), "b was not restored"
        self.same_on_every_rank(its, hist)
        return its, hist, self.gather(D.download("x"))

    def solve_single(self, b, x0, solver="pcg", **kw):
        R = self.R
        R.upload(0, "b", b)
        R.upload(0, "x", x0)
        its, hist = (R.pcg if solver == "pcg" else R.fgmres)(self.tol, **kw)
        return its, hist, R.download(0, "x")

    def compare(self, got, ref, b, solver, what, margin=True):
        """rank 0: the comparison rule of the module docstring"""
        from fgmres_restatement import assert_margin, true_relres
        (its, hist, x), (its1, hist1, x1) = got, ref
        print(f"{what}: {its} iterations (single GPU {its1})\n  dist   {hist}\n  single {hist1}", flush=True)
        if margin:
            assert_margin(hist1, self.tol, what)
        assert its == its1, (its, its1)
        assert np.allclose(hist, hist1, rtol=1e-6, atol=0), (hist, hist1)
        dx = np.linalg.norm(x - x1)
        assert dx <= 1e-6 * np.linalg.norm(x1), (dx, np.linalg.norm(x1))
        if margin:
            tr = true_relres(self.H, x, b)
            print(f"  true residual {tr:.3e} (tol {self.tol:g})", flush=True)
            assert tr < (10 * self.tol if solver == "pcg" else self.tol), tr

    def close(self):
        self.D.close()
        self.comm.close()
        if self.R is not None:
            self.R.close()


# ---- scenarios (each runs on every rank; rank 0 compares) -----------------------------------
def _sc_solve(c):
    """A full solve from x0 = 0 against the single-GPU solver."""
    cfg = c.cfg
    solver = cfg.get("solver", "pcg")
    kw = {"restart": cfg["restart"]} if solver == "fgmres" else {}
    b, x0 = c.rhs(cfg.get("seed", 1)), np.zeros(c.N)
    got = c.solve_dist(b, x0, solver, **kw)
    if c.rank == 0:
        c.compare(got, c.solve_single(b, x0, solver, **kw), b, solver, cfg["name"])


def _sc_one_sided(c):
    """b zero on rank 0's rows: a rank that tested its own ||b|| would return at once (or hang the others)."""
    b = c.rhs(c.cfg.get("seed", 1))
    ranges = [None] * c.world
    c.dist.all_gather_object(ranges, (c.rank, c.lo, c.hi))
    lo0, hi0 = next((lo, hi) for r, lo, hi in ranges if r == 0)
    b[lo0:hi0] = 0.0
    x0 = np.zeros(c.N)
    got = c.solve_dist(b, x0)
    assert got[0] > 0
    if c.rank == 0:
        c.compare(got, c.solve_single(b, x0), b, "pcg", "one-sided right-hand side")


def _sc_zero_rhs(c):
    solver = c.cfg.get("solver", "pcg")
    kw = {"restart": 20} if solver == "fgmres" else {}
    its, hist, x = c.solve_dist(np.zeros(c.N), np.ones(c.N), solver, **kw)
    assert its == 0 and len(hist) == 0 and not x.any()


def _sc_exact_guess(c):
    """r0 = 0 exactly (b = A 1 in small integers, x0 = 1): no iteration on any rank, relres 0, x
    untouched -- not the step length 0 / 0 and maxit cycles on NaN vectors."""
    import oracle
    from amg_amd._native import dptr
    b = np.zeros(c.N)
    oracle.load().ora_mv_mxy(C.byref(c.H.level(0).A), dptr(np.ones(c.N)), dptr(b))
    assert b.any()
    its, hist, x = c.solve_dist(b, np.ones(c.N))
    assert its == 0 and len(hist) == 0
    assert np.array_equal(_u64(x), _u64(np.ones(c.N)))
    c.D.upload("b", b[c.lo:c.hi])
    c.D.upload("x", np.ones(c.hi - c.lo))
    n_it, rel = C.c_int(-1), C.c_double(-1.0)
    assert c.A.lib().sss_hip_dist_pcg(c.D.d, c.tol, 100, C.byref(n_it), C.byref(rel), None, 0) == 0
    assert n_it.value == 0 and rel.value == 0.0


def _sc_nonfinite_rhs(c):
    """One NaN in b, on rank 0's rows only: the other ranks see it in the reduced ||b|| alone.  Every
    rank returns ERROR_SOLVER_EXIT in the same iteration, x the initial guess, b back as it was."""
    b, x0 = c.rhs(), c.rhs(2)
    ranges = [None] * c.world
    c.dist.all_gather_object(ranges, (c.rank, c.lo, c.hi))
    lo0, hi0 = next((lo, hi) for r, lo, hi in ranges if r == 0)
    b[(lo0 + hi0) // 2] = np.nan
    c.D.upload("b", b[c.lo:c.hi])
    c.D.upload("x", x0[c.lo:c.hi])
    its, rel = C.c_int(-1), C.c_double(-1.0)
    rc = c.A.lib().sss_hip_dist_pcg(c.D.d, c.tol, 100, C.byref(its), C.byref(rel), None, 0)
    got = [None] * c.world
    c.dist.all_gather_object(got, (rc, its.value))
    assert all(g == got[0] for g in got), got
    assert rc == -49 and its.value <= 1, (rc, its.value)   # ERROR_SOLVER_EXIT
    assert np.array_equal(_u64(c.D.download("x")), _u64(x0[c.lo:c.hi]))
    assert np.array_equal(_u64(c.D.download("b")), _u64(b[c.lo:c.hi]))
    with pytest.raises(RuntimeError):
        c.D.pcg(c.tol)


def _sc_pcg_edges(c):
    """maxit = 3; hist_cap = 1 and hist = NULL through raw ctypes."""
    from amg_amd._native import dptr
    lib = c.A.lib()
    b, x0 = c.rhs(), np.zeros(c.N)
    full = c.solve_dist(b, x0)
    got = c.solve_dist(b, x0, maxit=3)
    assert got[0] == 3 and len(got[1]) == 3
    if c.rank == 0:
        ref = c.solve_single(b, x0, maxit=3)
        assert ref[0] == 3
        c.compare(got, ref, b, "pcg", "maxit 3", margin=False)
    for hist in (np.full(3, -1.0), None):
        c.D.upload("b", b[c.lo:c.hi])
        c.D.upload("x", x0[c.lo:c.hi])
        its, rel = C.c_int(), C.c_double()
        rc = lib.sss_hip_dist_pcg(c.D.d, c.tol, 100, C.byref(its), C.byref(rel), None if hist is None else dptr(hist),
                                  1 if hist is not None else 0)
        assert rc == 0 and its.value == full[0]
        # (world 2: two-term sums, so a repeated solve is bitwise the first)
        assert rel.value == full[1][-1]
        if hist is not None:   # only hist_cap entries are written
            assert hist[0] == full[1][0] and hist[1] == hist[2] == -1.0
        x = c.gather(c.D.download("x"))
        assert np.array_equal(_u64(x), _u64(full[2]))


def _sc_engine_state(c):
    """One cycle on b = x = 1 right after a pcg is bitwise a fresh single-GPU engine's: nothing stale
    is left of the fused residual halves, and b came back."""
    c.solve_dist(c.rhs(), np.zeros(c.N))
    own = c.hi - c.lo
    c.D.upload("b", np.ones(own))
    c.D.upload("x", np.ones(own))
    c.D.cycle()
    x = c.gather(c.D.download("x"))
    if c.rank == 0:
        c.R.upload(0, "b", np.ones(c.N))
        c.R.upload(0, "x", np.ones(c.N))
        c.R.cycle()
        x1 = c.R.download(0, "x")
        assert np.array_equal(_u64(x), _u64(x1)), f"max |dx| = {np.max(np.abs(x - x1))}"


def _sc_deterministic(c):
    """World 2: a two-term sum does not depend on its order, so two solves agree bitwise."""
    b, x0 = c.rhs(), np.zeros(c.N)
    i1, h1, x1 = c.solve_dist(b, x0)
    i2, h2, x2 = c.solve_dist(b, x0)
    assert i1 == i2 and np.array_equal(h1, h2) and np.array_equal(_u64(x1), _u64(x2))


def _sc_fgmres_edges(c):
    """Zero right-hand side; restart = 0 on every rank; maxit = 4 with restart 3."""
    lib = c.A.lib()
    _sc_zero_rhs(c)
    its, rel = C.c_int(), C.c_double()
    assert lib.sss_hip_dist_fgmres(c.D.d, c.tol, 0, 100, C.byref(its), C.byref(rel), None, 0) == -12   # ERROR_INPUT_PAR
    with pytest.raises(RuntimeError):
        c.D.fgmres(c.tol, restart=0)
    b, x0 = c.rhs(), np.zeros(c.N)
    got = c.solve_dist(b, x0, "fgmres", restart=3, maxit=4)
    assert got[0] == 4
    if c.rank == 0:
        ref = c.solve_single(b, x0, "fgmres", restart=3, maxit=4)
        assert ref[0] == 4
        c.compare(got, ref, b, "fgmres", "maxit 4, restart 3", margin=False)


def _sc_same_solver(c):
    """World 1: the partitioned FGMRES is the single-GPU FGMRES -- one loop, the same kernels on the same
    rows, a sum over one rank -- so the count, the history and x agree bit for bit, and both restore b."""
    assert c.world == 1
    restart = c.cfg["restart"]
    b, x0 = c.rhs(c.cfg.get("seed", 1)), np.zeros(c.N)
    its, hist, x = c.solve_dist(b, x0, "fgmres", restart=restart)   # asserts that b came back
    its1, hist1, x1 = c.solve_single(b, x0, "fgmres", restart=restart)
    print(f"{c.cfg['name']}: {its} iterations (single GPU {its1})\n  dist   {hist}\n  single {hist1}", flush=True)
    assert its > 0 and its == its1, (its, its1)
    assert np.array_equal(_u64(hist), _u64(hist1)), np.flatnonzero(_u64(hist) != _u64(hist1))
    assert np.array_equal(_u64(x), _u64(x1)), f"max |dx| = {np.max(np.abs(x - x1))}"
    assert np.array_equal(_u64(c.R.download(0, "b")), _u64(b)), "the single-GPU b was not restored"


SCENARIOS = {f.__name__[4:]: f for f in (_sc_solve, _sc_one_sided, _sc_zero_rhs, _sc_exact_guess, _sc_nonfinite_rhs,
                                          _sc_pcg_edges, _sc_engine_state, _sc_deterministic, _sc_fgmres_edges,
                                          _sc_same_solver)}


def _worker(rank, world, port, cfg, errq):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch  # noqa: F401
        import torch.distributed as dist

        dist.init_process_group("gloo", rank=rank, world_size=world)
        c = _Ctx(rank, world, cfg)
        SCENARIOS[cfg.get("scenario", "solve")](c)
        if cfg.get("transport") == "rccl":
            graph = os.environ.get("SSS_HIP_DIST_GRAPH", "1") != "0"
            assert c.D.level_flags(0)["cycle_graph"] == graph   # the replayed graph ran inside the loop (or did not)
        c.close()
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        import traceback
        errq.put(f"rank {rank}: {e!r}\n{traceback.format_exc()}")


def _run(world, **cfg):
    import torch.multiprocessing as mp

    cfg.setdefault("name", " ".join(f"{k}={v}" for k, v in cfg.items() if k != "parts"))
    ctx = mp.get_context("spawn")
    errq = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, cfg, errq)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=JOIN_TIMEOUT)
    hung = [p for p in procs if p.is_alive()]
    for p in hung:
        p.kill()
        p.join()
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not hung, f"{len(hung)} rank(s) still waiting after {JOIN_TIMEOUT} s\n" + "\n".join(errs)
    assert not errs, "\n".join(errs)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]


# ---- PCG ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,smoother,inner_from,agg", [
    (7, 24, "hybrid", 2, 100),     # level 0 exact red-black GS-CF, two-stage from level 2
    (7, 24, "jacobi", 0, 100),     # two-stage everywhere
    (27, 14, "jacobi", 2, 100),    # 27-point: C/F-Jacobi forms only
])
def test_pcg_equals_single_gpu(kind, n, smoother, inner_from, agg):
    _run(2, kind=kind, n=n, smoother=smoother, inner_from=inner_from, agg=agg)


@pytest.mark.parametrize("world,kind,n,smoother,agg", [
    (4, 7, 32, "hybrid", 60), (8, 7, 32, "hybrid", 60), (4, 27, 16, "jacobi", 40)])
def test_pcg_multi_peer(world, kind, n, smoother, agg, monkeypatch):
    """Several peers per rank, the halo-overlap split launches on (SSS_HIP_OVERLAP=2): q = A p goes
    through the split launch with p's halo in between."""
    monkeypatch.setenv("SSS_HIP_OVERLAP", "2")
    _run(world, kind=kind, n=n, smoother=smoother, agg=agg)


def test_pcg_from_partition_files(tmp_path):
    import amg_amd as A
    from conftest import build_hierarchy, quiet_ctx
    H = build_hierarchy(A.generate(7, 24), quiet_ctx)
    A.part_save(H, 2, tmp_path / "part", 100)
    H.close()
    _run(2, kind=7, n=24, smoother="hybrid", agg=100, parts=str(tmp_path / "part"))


@pytest.mark.parametrize("graph", ["0", None], ids=["eager", "graph"])
def test_pcg_rccl_single_rank(graph, monkeypatch):
    """RCCL on the one GPU a test box has: the in-place device reductions (ncclAllReduce on the engine
    stream, scalars never leaving the device but for the stop test) and, by default, the captured
    cycle replayed inside the loop.  RCCL between two real peers cannot be tested on one GPU."""
    if graph is None:
        monkeypatch.delenv("SSS_HIP_DIST_GRAPH", raising=False)
    else:
        monkeypatch.setenv("SSS_HIP_DIST_GRAPH", graph)
    _run(1, kind=7, n=24, smoother="hybrid", agg=100, transport="rccl")


def test_pcg_one_sided_rhs():
    _run(2, kind=7, n=24, smoother="hybrid", agg=100, scenario="one_sided")


def test_pcg_zero_rhs():
    _run(2, kind=7, n=24, smoother="hybrid", agg=100, scenario="zero_rhs")


def test_pcg_exact_initial_guess():
    _run(2, kind=7, n=24, smoother="hybrid", agg=100, scenario="exact_guess")


def test_pcg_nonfinite_rhs():
    _run(2, kind=7, n=24, smoother="hybrid", agg=100, scenario="nonfinite_rhs")


def test_pcg_stop_and_history_edges():
    _run(2, kind=7, n=24, smoother="hybrid", agg=100, scenario="pcg_edges")


def test_pcg_engine_state():
    _run(2, kind=7, n=24, smoother="hybrid", agg=100, scenario="engine_state")


def test_pcg_deterministic():
    _run(2, kind=7, n=24, smoother="hybrid", agg=100, scenario="deterministic")


# ---- FGMRES ---------------------------------------------------------------------------------
@pytest.mark.parametrize("world,restart", [(2, 20), (2, 3), (4, 20), (4, 3)])
def test_fgmres_convdiff(world, restart):
    """Nonsymmetric convection-diffusion 16^3 (4096 rows), Peclet 2; restart 3 restarts several times."""
    _run(world, kind="convdiff", n=16, smoother="jacobi", agg=100, solver="fgmres", restart=restart)


def test_fgmres_poisson():
    _run(2, kind=7, n=24, smoother="hybrid", agg=100, solver="fgmres", restart=20)


def test_fgmres_edges():
    _run(2, kind="convdiff", n=16, smoother="jacobi", agg=100, solver="fgmres", scenario="fgmres_edges")


@pytest.mark.parametrize("kind,n,smoother,restart", [
    ("convdiff", 11, "jacobi", 3),     # 1331 own rows: odd, every basis column padded to even
    ("convdiff", 11, "jacobi", 20),
    ("convdiff", 16, "jacobi", 3),     # several restarts
    ("convdiff", 16, "jacobi", 20),
    (7, 24, "hybrid", 20),
])
@pytest.mark.parametrize("transport", ["host", "rccl"])
def test_fgmres_world1_is_the_single_gpu_solver(transport, kind, n, smoother, restart):
    """Both engines run fgmres_solve: at world 1 their results are the same bits."""
    _run(1, kind=kind, n=n, smoother=smoother, agg=100, solver="fgmres", restart=restart, transport=transport,
         scenario="same_solver")
