"""GPU: SuiteSparse Matrix Market inputs through the reference's own ingest (SSS_mat_read:
SSS_main.c:12-22, mmio_highlevel.h:10-305) -- BASELINE.json configs[0] (nos5 via ./amg) and
configs[3] (G3_circuit, the load-balance path), when the files are supplied.

The SuiteSparse files are not in this repository (no network; SURVEY.md 8(c): "the harness must skip
them if absent").  Put nos5.mtx and/or G3_circuit.mtx in $SSS_MTX_DIR and these tests run them; without
the files they skip.  1138_bus (the reference's only in-tree matrix, tests/golden/) always runs the same
checks, so the path itself is exercised on every GPU run.

Per file:
- parity mode (exact GS-CF, the reference's CG(beta=1)+GMRES coarse solve): x bitwise the oracle's
  restatement of the reference (every V-cycle up to tol on small inputs; the first two V-cycles on
  inputs above 200K rows, where the oracle's serial solve would take minutes), relres within 1e-13;
- throughput mode: below tol within the reference-semantics iteration count + 2 (SURVEY.md 8(c)
  ladder), that count measured by the parity engine on the same operator;
- the drop-in CLI (amg file.mtx, the reference's main): the printed relres column equals the oracle's
  history at %13.6e on small inputs;
- bench.py --full --mtx: one GPU run of the whole bench line on the file (small inputs).
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import amg_amd as A
from conftest import BUS_MTX, ROOT, build_hierarchy, oracle_solve, quiet_ctx
from test_gpu_parity import _gpu_history

pytestmark = pytest.mark.gpu

SMALL = 200_000   # rows up to which the oracle runs the whole solve


def _path(name: str) -> Path:
    if name == "1138_bus":
        return BUS_MTX
    d = os.environ.get("SSS_MTX_DIR")
    p = Path(d) / f"{name}.mtx" if d else None
    if p is None or not p.is_file():
        pytest.skip(f"{name}.mtx not supplied (set SSS_MTX_DIR to a directory holding it)")
    return p


@pytest.fixture(scope="module", params=["1138_bus", "nos5", "G3_circuit"])
def mtx(request):
    p = _path(request.param)
    M = A.read_mtx(p)
    H = build_hierarchy(M, quiet_ctx)
    A.lib().SSS_mat_destroy(__import__("ctypes").byref(M))
    yield request.param, p, H
    H.close()


def test_mtx_parity_bitwise(mtx):
    name, _, H = mtx
    n = H.level(0).A.num_rows
    small = n <= SMALL
    saved = H.mg.pars.max_it
    if not small:
        H.mg.pars.max_it = 2
    try:
        b, x_r = np.ones(n), np.ones(n)
        rtn, rel_r, _ = oracle_solve(H, b, x_r)
    finally:
        H.mg.pars.max_it = saved
    rel_g, x_g = _gpu_history(H, max_it=len(rel_r))
    assert len(rel_g) == len(rel_r)
    assert np.array_equal(x_g.view(np.uint64), x_r.view(np.uint64)), name
    assert np.allclose(rel_g, rel_r, rtol=1e-13, atol=0)
    if small:
        assert rel_r[-1] < H.pars.tol or len(rel_r) == H.pars.max_it


def test_mtx_throughput_ladder(mtx):
    name, _, H = mtx
    rel_p, x_p = _gpu_history(H)   # reference semantics (bitwise the oracle's iterates)
    rel_t, x_t = _gpu_history(H, smoother="hybrid", coarse="direct")
    print(f"{name}: parity {len(rel_p)} iterations (relres {rel_p[-1]:.3e}), throughput {len(rel_t)} "
          f"(relres {rel_t[-1]:.3e})")
    if rel_p[-1] < H.pars.tol:
        assert rel_t[-1] < H.pars.tol
        assert len(rel_t) <= len(rel_p) + 2


def test_mtx_cli_table(mtx):
    """./amg file.mtx (SSS_main.c:121-159 semantics): its printed relres column is the oracle's."""
    name, p, H = mtx
    n = H.level(0).A.num_rows
    if n > SMALL:
        pytest.skip("the oracle's whole serial solve is checked on small inputs only")
    rtn, rel_r, _ = oracle_solve(H, np.ones(n), np.ones(n))
    exe = ROOT / "amg_amd" / "bin" / "amg"
    r = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [l.split("|") for l in r.stdout.splitlines() if l[:6].strip().isdigit() and "|" in l]
    assert [c[1].strip() for c in rows[1:]] == ["%.6e" % v for v in rel_r], name
    assert f"AMG iterations: {len(rel_r)}" in r.stdout or len(rel_r) == H.pars.max_it


def test_bench_mtx_line(mtx):
    """bench.py --mtx: the bench line on the file (one GPU), its iterations inside the ladder."""
    name, p, H = mtx
    if H.level(0).A.num_rows > SMALL:
        pytest.skip("the full bench line on large files is a bench run, not a test")
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--mtx", str(p), "--steps", "3", "--warmup", "1",
                        "--full", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["config"]["workload"] == f"mtx_{p.stem}"
    assert rec["config"]["rows"] == H.level(0).A.num_rows and rec["value"] > 0
    conv = rec["config"]["reference_convergence"]
    assert conv and conv["source"].startswith("this run")
    if conv["ladder"] != "ok":   # the reference's own coarse solve may fail to reach tol (1138_bus does not)
        assert rec["parity_mode"]["final_relres"] >= H.pars.tol
